// Host orchestration of the HIP encode path behind SaveImage (include/jxlfiletypeio.h).
//
// Mirrors EncoderWriteImage (reference: src/JxlFileTypeIO/Encoder/JxlEncoder.cpp:147-392): parameter checks (:155-158),
// progress / cancellation checkpoints (:79-89,162,169,242,253,312,340-344,362), pixel-format analysis (:33-77),
// channel conversion (PixelFormatConversion.cpp:16-121), container output with Exif / XMP boxes (:201,284-310) through
// the host's Write callback in chunks of at most 64 KiB (OutputProcessor.cpp:16,87,134-151).  The arithmetic the
// reference delegates to libjxl (JxlEncoderAddImageFrame :128, JxlEncoderFlushInput :367) runs in encode_kernels.hip.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <atomic>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>
#include "../../include/jxlfiletypeio.h"
#include "enc_animation.h"
#include "enc_batch_layout.h"
#include "enc_types.h"
#include "host_parse.h"
#include "host_write.h"
#include "icc.h"
#include "kernels.h"
#include "modular_rules.h"

namespace jxlhip {

void LaunchEncAnalyze(const EncImage& im, hipStream_t s);
void LaunchEncFrontEnd(const EncImage& im, hipStream_t s);
void LaunchEncTokens(const EncImage& im, hipStream_t s);
void LaunchEncReverse(const EncImage& im, int which, hipStream_t s);
void LaunchEncSections(const EncImage& im, hipStream_t s);
void LaunchEncCompact(const EncImage& im, const uint64_t* dst_off, uint8_t* dst, int nsec, hipStream_t s);
void LaunchEncLossless(const EncImage& im, int stage, hipStream_t s);
void LaunchEncLosslessSearch(const EncImage& im, const LlSearch& ls, int stage, hipStream_t s);   // lossless_kernels.hip
void LaunchEncXyb(const EncImage& im, hipStream_t s);
void LaunchEncPackBgra(const EncImage& im, const uint8_t* src, int nch, hipStream_t s);
void LaunchEncVarblocks(const EncImage& im, hipStream_t s);
// batch forms of the serial kernels: every image of `ims` that the table lists, in one launch (encode_kernels.hip)
size_t EncReverseLds(uint32_t num_clusters, uint32_t num_ctx, int which);
int EncSectionsPerWg();
void LaunchEncReverseBatch(const EncImage* ims, const EncBatchTable& t, uint32_t units, int which, size_t lds, hipStream_t s);
void LaunchEncSectionsBatch(const EncImage* ims, const EncBatchTable& t, uint32_t units, hipStream_t s);
void LaunchEncGlobalAlphaBatch(const EncImage* ims, const EncBatchTable& t, hipStream_t s);
void LaunchEncLlSectionsBatch(const EncImage* ims, const EncBatchTable& t, uint32_t units, size_t lds, hipStream_t s);
void LaunchEncCompactBatch(const EncImage* ims, const EncBatchTable& t, uint32_t units, const uint64_t* dst_off, uint8_t* dst, hipStream_t s);
// distance_kernels.hip
void LaunchDistMask(const DistMap& dm, hipStream_t s);
void LaunchDistCells(const DistMap& dm, hipStream_t s);
void LaunchDistCorrect(const EncImage& im, const float* cell, const int32_t* q0, float tau, float p_up, float p_down, bool allow_down, hipStream_t s);

namespace {

struct EncFail : std::runtime_error {
  EncoderStatus status;
  EncFail(EncoderStatus st, const std::string& m) : std::runtime_error(m), status(st) {}
};
#define ENC_HIP(expr)                                                                                                   \
  do {                                                                                                                  \
    hipError_t e_ = (expr);                                                                                             \
    if (e_ == hipErrorOutOfMemory) throw EncFail(EncoderStatus_OutOfMemory, "out of device memory");                    \
    if (e_ != hipSuccess) throw EncFail(EncoderStatus_EncodeError, std::string(#expr) + ": " + hipGetErrorString(e_));  \
  } while (0)

void SetEncErr(ErrorInfo* e, const char* msg) {
  if (!e || !msg) return;
  size_t n = strlen(msg);
  if (n == 0) return;
  if (n > 255) n = 255;
  memcpy(e->errorMessage, msg, n);
  e->errorMessage[n] = 0;
}

// device allocations of one SaveImage call
struct Arena {
  std::vector<void*> ptrs;
  ~Arena() { for (void* p : ptrs) (void)hipFree(p); }
  template <class T> T* Get(size_t count, bool zero = false) {
    void* p = nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(T), 256);
    ENC_HIP(hipMalloc(&p, bytes));
    ptrs.push_back(p);
    if (zero) ENC_HIP(hipMemset(p, 0, bytes));
    return (T*)p;
  }
  template <class T> T* Counter(EncCounterKind, size_t count) { return Get<T>(count); }   // (a batch keeps the kinds apart: enc_batch_layout.h)
  template <class T> T* Upload(const std::vector<T>& v) {
    T* p = Get<T>(std::max<size_t>(v.size(), 1));
    if (!v.empty()) ENC_HIP(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return p;
  }
};

// JXLHIP_ENC_TIMING=1: wall time of the encoder's phases on stderr (host + device, synchronised at each checkpoint)
struct PhaseClock {
#ifdef JXLHIP_EXPERIMENTS
  bool on = getenv("JXLHIP_ENC_TIMING") != nullptr;
#else
  bool on = false;
#endif
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void Lap(const char* what) {
    if (!on) return;
    (void)hipDeviceSynchronize();
    const auto n = std::chrono::steady_clock::now();
    fprintf(stderr, "[enc] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
    t = n;
  }
};

// Device time of the encoder's kernel groups, always recorded (a pair of HIP events on the group's own stream; the streams overlap,
// so the groups can add up to more than the call): what bench.py's encode workload reads through jxlhip_last_save_stage_times.
struct StageMarks {
  struct M { const char* name; hipEvent_t a, b; };
  std::vector<M> marks;
  ~StageMarks() { for (auto& m : marks) { (void)hipEventDestroy(m.a); (void)hipEventDestroy(m.b); } }
  size_t Begin(const char* name, hipStream_t s) {
    M m{name, nullptr, nullptr};
    if (hipEventCreate(&m.a) != hipSuccess || hipEventCreate(&m.b) != hipSuccess) return (size_t)-1;
    (void)hipEventRecord(m.a, s);
    marks.push_back(m);
    return marks.size() - 1;
  }
  void End(size_t i, hipStream_t s) { if (i < marks.size()) (void)hipEventRecord(marks[i].b, s); }
  void Publish(std::vector<std::pair<const char*, float>>* out) {
    out->clear();
    for (auto& m : marks) {
      float ms = 0.f;
      if (hipEventSynchronize(m.b) == hipSuccess && hipEventElapsedTime(&ms, m.a, m.b) == hipSuccess) out->push_back({m.name, ms});
    }
  }
};
thread_local std::vector<std::pair<const char*, float>> g_last_save_stages;

// What the closed loop of this thread's last SaveImage measured (jxlhip_last_save_distances); evaluations == 0: it did not run
struct LastDistances {
  std::vector<float> cells;   // of the evaluation whose field was written
  int32_t evaluations = 0, over_first = 0, over_emitted = 0;
  float target = 0.f;
};
thread_local LastDistances g_last_dist;

// The constants of the distance map and of the loop (DESIGN.md §2 states them and why)
constexpr float kDistA0 = 0.02f, kDistK = 1.0f;
constexpr float kDistS[3] = {8.0f, 1.0f, 0.5f};
constexpr float kLoopPUp = 0.7f, kLoopPDown = 0.2f;

DistMap MakeDistMap(int32_t w, int32_t h) {
  DistMap dm;
  memset(&dm, 0, sizeof(dm));
  dm.w = w; dm.h = h; dm.w8 = (w + 7) / 8; dm.h8 = (h + 7) / 8;
  dm.a0 = kDistA0; dm.k = kDistK;
  for (int c = 0; c < 3; c++) dm.s2[c] = kDistS[c] * kDistS[c];
  return dm;
}

void Progress(ProgressProc progress, int percent) {
  if (progress && !progress(percent)) throw EncFail(EncoderStatus_UserCanceled, "");   // Encoder/JxlEncoder.cpp:79-89
}

}  // namespace

// The fixed MA tree of this encoder, in decode (breadth-first) order; leaf order = context ids of EncLeaf.  (Not file-local: the
// test library's self tests serialise it, csrc/selftest.cc.)  cfl_maps: the frame codes fitted chroma-from-luma maps, so their leaf
// predicts like the LF channels do instead of being a constant; shape and leaf numbering are the same.
std::vector<EncTreeNode> MakeEncoderTree(uint32_t nlf, bool cfl_maps) {
  auto split = [](int prop, int32_t v) { return EncTreeNode{prop, v, 0, 0, 1}; };
  auto leaf = [](int pred, int32_t offset = 0) { return EncTreeNode{-1, 0, pred, offset, 1}; };
  std::vector<EncTreeNode> t;
  t.push_back(split(1, (int32_t)(3 * nlf + kNumQuantTables)));   // 0: stream > LF + metadata + quant-table streams ? alpha : 2
  t.push_back(leaf(5));                                          // 1: alpha of a pass group              (kLeafAlpha)
  t.push_back(split(1, (int32_t)(2 * nlf)));                     // 2: HF metadata (3) : 4
  t.push_back(split(0, 2));                                      // 3: channel 3 = sharpness (5) : 6
  t.push_back(split(1, 0));                                      // 4: LF coefficients (7) : global alpha (8)
  t.push_back(leaf(0, 4));                                       // 5: EPF sharpness, constant 4            (kLeafSharp)
  t.push_back(split(0, 1));                                      // 6: channel 2 = block info (9) : chroma-from-luma maps (10)
  t.push_back(split(0, 1));                                      // 7: channel 2 = B (11) : 12
  t.push_back(leaf(5));                                          // 8: alpha coded in the global section   (kLeafAlphaGlobal)
  t.push_back(split(2, 0));                                      // 9: row 1 = quant field (13) : row 0 = strategies (14)
  t.push_back(leaf(cfl_maps ? 5 : 0));                           // 10: chroma-from-luma maps: constant 0, fitted: gradient (kLeafCfl)
  t.push_back(leaf(5));                                          // 11: LF of B                            (kLeafLfB)
  t.push_back(split(0, 0));                                      // 12: channel 1 = X (15) : channel 0 = Y (16)
  t.push_back(leaf(1));                                          // 13: quant field row, West predictor    (kLeafQf)
  t.push_back(leaf(0));                                          // 14: strategy row, constant 0 (DCT8)    (kLeafStrategy)
  t.push_back(leaf(5));                                          // 15: LF of X                            (kLeafLfX)
  t.push_back(leaf(5));                                          // 16: LF of Y                            (kLeafLfY)
  return t;
}
std::vector<EncTreeNode> MakeEncoderTree(uint32_t nlf) { return MakeEncoderTree(nlf, false); }

namespace {

int32_t HResultToStatus(int32_t hr) {   // OutputProcessor.cpp:134-151
  if (hr >= 0) return EncoderStatus_Ok;
  if ((uint32_t)hr == 0x80004004u) return EncoderStatus_UserCanceled;
  if ((uint32_t)hr == 0x8007000Eu) return EncoderStatus_OutOfMemory;
  return EncoderStatus_WriteError;
}

EncCodeDev UploadCode(Arena& A, const EncCode& c) {
  EncCodeDev d;
  d.ctx_map = A.Upload(c.ctx_map);
  d.freq = A.Upload(c.freq);
  d.start = A.Upload(c.start);
  d.rmap = A.Upload(c.rmap);
  d.num_clusters = c.num_clusters;
  d.num_ctx = (uint32_t)c.ctx_map.size();
  return d;
}

// Container + output through the host callbacks (always boxes, Encoder/JxlEncoder.cpp:201) in chunks of at most 64 KiB.
void EmitFile(const std::vector<uint8_t>& codestream, const EncoderImageMetadata* md, IOCallbacks* io, ProgressProc progress) {
  std::vector<uint8_t> file = WriteContainer(codestream, md->exif, md->exifSize, md->xmp, md->xmpSize);
  const size_t kChunk = 64 * 1024;   // OutputProcessor.cpp:16
  size_t done = 0;
  int last_pct = 30;
  while (done < file.size()) {
    const size_t n = std::min(kChunk, file.size() - done);
    const int32_t st = HResultToStatus(io->Write(file.data() + done, n));
    if (st != EncoderStatus_Ok) throw EncFail(st, st == EncoderStatus_WriteError ? "the output stream rejected a write" : "");
    done += n;
    const int pct = 30 + (int)(60.0 * done / file.size()) / 5 * 5;   // 30 -> 90 in steps of 5 (:340-344)
    if (pct > last_pct) { Progress(progress, pct); last_pct = pct; }
  }
  Progress(progress, 95);
}

// Where the pixels of a save come from and what the headers say about them: the BGRA8 surface of SaveImage (8-bit integers, sRGB), or
// the samples of jxlhip_save_pixels, already checked (CheckPixels).
struct EncSource {
  const BitmapData* bmp = nullptr;
  const JxlHipPixels* px = nullptr;
  uint32_t bits = 8, exp_bits = 0;          // as EncImageInfo
  uint32_t primaries = 1, transfer = 13;
  bool pq = false;
  uint32_t width() const { return bmp ? bmp->width : px->width; }
  uint32_t height() const { return bmp ? bmp->height : px->height; }
  size_t sample_bytes() const { return exp_bits == 8 ? 4 : (bits > 8 ? 2 : 1); }
  bool deep() const { return bits > 8; }    // more than 8 bits per sample, floats included
  void Describe(EncImageInfo& ii) const {
    ii.bits = bits; ii.exp_bits = exp_bits; ii.primaries = primaries; ii.transfer = transfer; ii.pq_intensity = pq;
  }
};

void Inv3(const double m[9], double o[9]) {
  const double d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
  o[0] = (m[4] * m[8] - m[5] * m[7]) / d; o[1] = (m[2] * m[7] - m[1] * m[8]) / d; o[2] = (m[1] * m[5] - m[2] * m[4]) / d;
  o[3] = (m[5] * m[6] - m[3] * m[8]) / d; o[4] = (m[0] * m[8] - m[2] * m[6]) / d; o[5] = (m[2] * m[3] - m[0] * m[5]) / d;
  o[6] = (m[3] * m[7] - m[4] * m[6]) / d; o[7] = (m[1] * m[6] - m[0] * m[7]) / d; o[8] = (m[0] * m[4] - m[1] * m[3]) / d;
}

// jxlhip_save_pixels: geometry + upload.  The channels are as stated (nothing is analysed); the rows are packed on the way up, so
// the device rows are tight whatever stride the caller's memory has (what the loaders of encode_kernels.hip rely on).  8-bit samples
// become the BGRA8 surface of SaveImage on the device, and every 8-bit path - the byte-keyed lossless search included - runs as it
// does for SaveImage.
// What the stated channels and colour encoding mean for the kernels, once the samples are on the device: `d_src` holds them in tight
// rows, `d_bgra` is room for the BGRA8 surface of 8-bit input (deeper input: unused).  im has its geometry.
void SetPixelSource(const EncSource& src, const uint8_t* d_src, uint8_t* d_bgra, EncImage& im, hipStream_t s) {
  const JxlHipPixels& px = *src.px;
  const uint32_t w = px.width;
  const int nch = px.num_channels;
  const size_t row = (size_t)w * nch * src.sample_bytes();
  im.gray = nch < 3;
  im.has_alpha = (nch & 1) ? 0 : 1;
  im.transfer = src.transfer == 8 ? kTransferLinear : (src.transfer == 1 ? kTransfer709 : (src.transfer == 16 ? kTransferPq : kTransferSrgb));
  if (!im.gray && (src.primaries != 1 || src.pq)) {
    // linear samples of the space's primaries, relative to its intensity target -> linear sRGB relative to 255 nits
    static const double kSrgb[3][2] = {{0.639998686, 0.330010138}, {0.300003784, 0.600003357}, {0.150002046, 0.059997204}};
    static const double kP3[3][2] = {{0.680, 0.320}, {0.265, 0.690}, {0.150, 0.060}}, k2100[3][2] = {{0.708, 0.292}, {0.170, 0.797}, {0.131, 0.046}};
    const double white[2] = {0.3127, 0.3290};
    double from_srgb[9], to_srgb[9];
    if (!MatrixFromLinearSrgb(src.primaries == 11 ? kP3 : (src.primaries == 9 ? k2100 : kSrgb), white, from_srgb))
      throw EncFail(EncoderStatus_EncodeError, "the colour encoding's primaries have no matrix");
    Inv3(from_srgb, to_srgb);
    const double sc = src.pq ? 10000.0 / 255.0 : 1.0;
    for (int k = 0; k < 9; k++) im.icc_to_srgb[k] = (float)(to_srgb[k] * sc);
    im.use_matrix = 1;
  }
  if (src.deep()) {
    im.bgra = d_src; im.stride = (int64_t)row;
    im.src_nch = nch;
    im.src_type = px.sample_type;
    im.sample_scale = 1.0f / (float)((1u << src.bits) - 1);
  } else {
    im.bgra = d_bgra; im.stride = (int64_t)w * 4;
    LaunchEncPackBgra(im, d_src, nch, s);
  }
}

void BeginPixels(const EncSource& src, Arena& A, EncImage& im, ProgressProc progress) {
  const JxlHipPixels& px = *src.px;
  const uint32_t w = px.width, h = px.height;
  SetEncGeometry(w, h, im);
  const size_t row = (size_t)w * px.num_channels * src.sample_bytes();
  uint8_t* d_src = A.Get<uint8_t>(row * h);
  ENC_HIP(hipMemcpy2D(d_src, row, px.data, px.stride_bytes, row, h, hipMemcpyHostToDevice));
  SetPixelSource(src, d_src, src.deep() ? nullptr : A.Get<uint8_t>((size_t)w * 4 * h), im, nullptr);
  Progress(progress, 5);
}

// Geometry + upload + pixel-format analysis shared by the lossy and the lossless path (Encoder/JxlEncoder.cpp:33-77).
void BeginImage(const EncSource& src, const EncoderImageMetadata* md, Arena& A, EncImage& im, ProgressProc progress) {
  if (src.px) return BeginPixels(src, A, im, progress);
  const BitmapData* bmp = src.bmp;
  const uint32_t w = bmp->width, h = bmp->height;
  if (!w || !h || !bmp->scan0 || bmp->stride < (uint64_t)w * 4) throw EncFail(EncoderStatus_EncodeError, "invalid bitmap");
  SetEncGeometry(w, h, im);
  uint8_t* d_bgra = A.Get<uint8_t>((size_t)bmp->stride * h);
  ENC_HIP(hipMemcpy(d_bgra, bmp->scan0, (size_t)bmp->stride * h, hipMemcpyHostToDevice));
  im.bgra = d_bgra; im.stride = (int64_t)bmp->stride;
  im.transfer = kTransferSrgb;
  im.flags = A.Get<uint32_t>(4, true);
  LaunchEncAnalyze(im, nullptr);
  uint32_t flags[2] = {0, 0};
  ENC_HIP(hipMemcpy(flags, im.flags, sizeof(flags), hipMemcpyDeviceToHost));
  im.gray = flags[0] ? 0 : 1;       // every pixel r == g == b and no ICC profile: one colour channel (:67-70)
  if (md->iccProfile && md->iccProfileSize) im.gray = 0;   // an RGB profile must keep describing RGB samples (:71-75)
  im.has_alpha = flags[1] ? 1 : 0;  // some pixel a < 255 (:54-57)
  Progress(progress, 5);
}

// A frame of an animation: its headers speak of `canvas`, it lies at `at`, and no image header is written in front of it.
struct FrameOnCanvas { EncImageInfo canvas; EncFramePlacement at; };

std::vector<uint8_t> AssembleLossless(const EncImage& im, const EncSource& src, const EncoderImageMetadata* md, BitWriter& lf_global, const uint8_t* packed,
                                      const uint64_t* off, const uint64_t* sec_bits, const FrameOnCanvas* on = nullptr);

// ANS-codes the groups' tokens (im.tok_ll) with `mcode`, gathers the sections and assembles the codestream behind the finished LfGlobal
// prefix.  The section buffers are allocated at the first call of a save and reused by the next.
std::vector<uint8_t> FinishLossless(EncImage& im, const EncSource& src, Arena& A, const EncCode& mcode, BitWriter& lf_global, const EncoderImageMetadata* md, hipStream_t s) {
  im.mcode = UploadCode(A, mcode);
  const int nsec = im.ng;
  if (!im.sec_bytes) {
    LayLosslessSections(A, im);
    ENC_HIP(hipMemset(im.sec_bits, 0, std::max<size_t>((size_t)nsec * 8, 256)));
    ENC_HIP(hipMemset(im.stream_state, 0, std::max<size_t>(EncNumStreamStates(im) * 4, 256)));
  } else {
    ENC_HIP(hipMemset(im.sec_bits, 0, std::max<size_t>((size_t)nsec * 8, 256)));
  }
  LaunchEncLossless(im, 1, s);
  std::vector<uint64_t> sec_bits(nsec);
  ENC_HIP(hipMemcpy(sec_bits.data(), im.sec_bits, sec_bits.size() * 8, hipMemcpyDeviceToHost));
  std::vector<uint64_t> off(nsec + 1, 0);
  for (int i = 0; i < nsec; i++) off[i + 1] = off[i] + ((sec_bits[i] + 7) >> 3);
  std::vector<uint8_t> packed(std::max<uint64_t>(off[nsec], 1));
  {
    uint64_t* d_off = A.Upload(off);
    uint8_t* d_packed = A.Get<uint8_t>(packed.size());
    LaunchEncCompact(im, d_off, d_packed, nsec, s);
    ENC_HIP(hipMemcpy(packed.data(), d_packed, packed.size(), hipMemcpyDeviceToHost));
  }
  ENC_HIP(hipGetLastError());
  return AssembleLossless(im, src, md, lf_global, packed.data(), off.data(), sec_bits.data());
}

// What the image headers say: size and channels of `im`, depth and colour encoding of `src`, the profile of `md`.
EncImageInfo DescribeImage(const EncImage& im, const EncSource& src, const EncoderImageMetadata* md, bool xyb) {
  EncImageInfo ii;
  ii.xsize = (uint32_t)im.w; ii.ysize = (uint32_t)im.h; ii.gray = im.gray; ii.alpha = im.has_alpha; ii.xyb = xyb;
  ii.icc = md->iccProfile; ii.icc_size = md->iccProfile ? md->iccProfileSize : 0;
  src.Describe(ii);
  return ii;
}

// The codestream of a Modular frame behind its finished LfGlobal prefix.  packed + off[g], sec_bits[g]: the coded section of group g.
// `on`: the frame alone, as a frame of an animation.
std::vector<uint8_t> AssembleLossless(const EncImage& im, const EncSource& src, const EncoderImageMetadata* md, BitWriter& lf_global, const uint8_t* packed,
                                      const uint64_t* off, const uint64_t* sec_bits, const FrameOnCanvas* on) {
  const bool single = im.ng == 1;
  const EncImageInfo ii = on ? on->canvas : DescribeImage(im, src, md, false);
  EncFrameInfo fi;
  fi.encoding = 1; fi.group_size_shift = 1; fi.gab = false; fi.epf_iters = 0;
  if (on) fi.at = on->at;
  BitWriter cs;
  if (!on) WriteCodestreamHeaders(ii, cs);
  WriteFrameHeader(ii, fi, cs);
  std::vector<std::vector<uint8_t>> sections;
  if (single) {
    lf_global.AppendBits(packed + off[0], sec_bits[0]);   // the channels of a frame that fits one group belong to the global stream
    sections.push_back(lf_global.Finish());
  } else {
    sections.push_back(lf_global.Finish());
    for (int g = 0; g < im.nlf; g++) sections.emplace_back();   // no channel is small enough for the LF groups
    sections.emplace_back();                                    // HfGlobal is empty in a Modular frame
    for (int g = 0; g < im.ng; g++) sections.emplace_back(packed + off[g], packed + off[g] + ((sec_bits[g] + 7) >> 3));
  }
  std::vector<uint32_t> sizes;
  for (auto& sec : sections) sizes.push_back((uint32_t)sec.size());
  WriteToc(sizes, cs);
  std::vector<uint8_t> codestream = cs.Finish();
  for (auto& sec : sections) codestream.insert(codestream.end(), sec.begin(), sec.end());
  return codestream;
}

// LfGlobal of the fixed lossless stream: tree on the channel index (leaf ids: channel 3, 2, 1, 0), the code of the channels' token
// histograms hist[4][kEncSyms], GlobalModular header.
void WriteLosslessFixedGlobal(const EncImage& im, const uint32_t* hist, BitWriter& lf_global, EncCode& mcode) {
  lf_global.Bool(true);   // default LF dequantisation factors (read for every frame encoding)
  lf_global.Bool(true);   // global MA tree
  {
    std::vector<EncTreeNode> t;
    t.push_back(EncTreeNode{0, 1, 0, 0, 1});     // 0: channel > 1 ? 1 : 2
    t.push_back(EncTreeNode{0, 2, 0, 0, 1});     // 1: channel > 2 ? 3 : 4
    t.push_back(EncTreeNode{0, 0, 0, 0, 1});     // 2: channel > 0 ? 5 : 6
    for (int i = 0; i < 4; i++) t.push_back(EncTreeNode{-1, 0, 5, 0, 1});   // gradient predictor leaves: channel 3, 2, 1, 0
    WriteTree(t, lf_global);
  }
  BuildAndWriteCode(hist, 4, 4, {}, lf_global, mcode);
  lf_global.Bool(true);   // use the global tree
  lf_global.Bool(true);   // default weighted-predictor parameters
  lf_global.U32(WV(0), WV(1), WB(4, 2), WB(8, 18), im.ll_rct ? 1 : 0);
  if (im.ll_rct) {
    lf_global.Write(2, 0);                                            // transform id 0: reversible colour transform
    lf_global.U32(WB(3), WB(6, 8), WB(10, 72), WB(13, 1096), 0);      // first channel
    lf_global.U32(WV(6), WB(2), WB(4, 2), WB(6, 10), 6);              // type 6: YCoCg-R
  }
}

// The stream of efforts 1..7: 256x256 groups, YCoCg-R for RGB, gradient predictor, one context per channel.  `progress` (may be
// null) sees 25 once the histograms are down.
std::vector<uint8_t> CodeLosslessFixed(EncImage& im, const EncSource& src, Arena& A, const EncoderImageMetadata* md, hipStream_t s, ProgressProc progress) {
  im.ll_nch = (im.gray ? 1 : 3) + im.has_alpha;
  im.ll_rct = im.gray ? 0 : 1;
  im.ll_tok_extra = 0;
  im.hist_mod = A.Get<uint32_t>(kNumEncLeaves * kEncSyms, true);
  LaunchEncLossless(im, 0, s);
  std::vector<uint32_t> hist(4 * kEncSyms);
  ENC_HIP(hipMemcpy(hist.data(), im.hist_mod, hist.size() * 4, hipMemcpyDeviceToHost));
  Progress(progress, 25);
  BitWriter lf_global;
  EncCode mcode;
  WriteLosslessFixedGlobal(im, hist.data(), lf_global, mcode);
  return FinishLossless(im, src, A, mcode, lf_global, md, s);
}

// ---- the searched stream of efforts 8 and 9 ("Lossless efforts 8 and 9")

// bits of a token histogram: zero-order entropy plus the extra bits of the hybrid-uint config (4, 2, 0), which the token determines
double TokenCost(const uint32_t* h) {
  uint64_t total = 0;
  for (uint32_t t = 0; t < kEncSyms; t++) total += h[t];
  double bits = 0;
  for (uint32_t t = 0; t < kEncSyms; t++) {
    if (!h[t]) continue;
    bits += (double)h[t] * std::log2((double)total / (double)h[t]);
    if (t >= 16) bits += (double)h[t] * (double)(2 + ((t - 16) >> 2));
  }
  return bits;
}

// An MA tree under construction: nodes point at their children, Flatten puts them in decode (breadth-first) order and numbers the
// leaves as the decoder will (context id = rank of the leaf in that order).
struct TreeBuilder {
  struct Node { int property; int32_t splitval; int pred; int gt, le; };
  std::vector<Node> nodes;
  int Leaf(int pred) { nodes.push_back(Node{-1, 0, pred, -1, -1}); return (int)nodes.size() - 1; }
  int Split(int property, int32_t v, int gt, int le) { nodes.push_back(Node{property, v, 0, gt, le}); return (int)nodes.size() - 1; }
  std::vector<EncTreeNode> Flatten(int root, std::vector<int>* ctx_of_node) const {
    std::vector<EncTreeNode> out;
    ctx_of_node->assign(nodes.size(), -1);
    std::vector<int> order{root};
    int leaves = 0;
    for (size_t k = 0; k < order.size(); k++) {
      const Node& n = nodes[order[k]];
      if (n.property < 0) { out.push_back(EncTreeNode{-1, 0, n.pred, 0, 1}); (*ctx_of_node)[order[k]] = leaves++; continue; }
      out.push_back(EncTreeNode{n.property, n.splitval, 0, 0, 1});
      order.push_back(n.gt);
      order.push_back(n.le);
    }
    return out;
  }
};

}  // namespace

// The thresholds of property 15 that split a channel's contexts at effort 9 (the oracle writer's), and the searched tree: the channel
// (a palette frame: palette against indices, see below), then, with `wp_ctx`, property 15 searched over the thresholds.  ctx[c][k]:
// context of channel c, bucket k = number of thresholds the property exceeds.  `palette`: 0 none; 1 a one-group frame, whose global
// stream holds the colours as channel 0 and the indices as channel 1; 2 a frame of several groups, whose colours are alone in the global
// stream (stream 0) and whose indices are channel 0 of every group's stream.  *palette_ctx: the colours' context.  (Not file-local:
// the test library's self tests serialise it, csrc/selftest.cc.)
extern const int32_t kWpCutsHost[kWpLeaves - 1] = {-80, -24, -8, -3, -1, 0, 2, 7, 23, 79};
std::vector<EncTreeNode> MakeLosslessSearchTree(int nch, const int32_t* pred, bool wp_ctx, int palette, uint8_t ctx[4][kWpLeaves + 1], int* palette_ctx) {
  TreeBuilder b;
  int leaf_of[4][kWpLeaves];
  int sub[4];
  for (int c = 0; c < nch; c++) {
    if (!wp_ctx) {
      sub[c] = b.Leaf(pred[c]);
      for (int k = 0; k < kWpLeaves; k++) leaf_of[c][k] = sub[c];
      continue;
    }
    struct R { static int Build(TreeBuilder& b, int lo, int hi, int pred, int* leaf_of) {   // thresholds [lo, hi)
      if (lo == hi) return leaf_of[lo] = b.Leaf(pred);
      const int mid = (lo + hi) / 2;
      const int gt = Build(b, mid + 1, hi, pred, leaf_of), le = Build(b, lo, mid, pred, leaf_of);
      return b.Split(15, kWpCutsHost[mid], gt, le);
    } };
    sub[c] = R::Build(b, 0, kWpLeaves - 1, pred[c], leaf_of[c]);
  }
  int root = sub[nch - 1];
  for (int c = nch - 2; c >= 0; c--) root = b.Split(0, c, root, sub[c]);   // channel > c ? the channels after c : c
  int pal_leaf = -1;
  if (palette) {
    pal_leaf = b.Leaf(pred[nch]);
    root = palette == 1 ? b.Split(0, 0, root, pal_leaf) : b.Split(1, 0, root, pal_leaf);
  }
  std::vector<int> ctx_of;
  std::vector<EncTreeNode> t = b.Flatten(root, &ctx_of);
  for (int c = 0; c < nch; c++)
    for (int k = 0; k < kWpLeaves; k++) ctx[c][k] = (uint8_t)ctx_of[leaf_of[c][k]];
  if (palette_ctx) *palette_ctx = palette ? ctx_of[pal_leaf] : -1;
  return t;
}

// The GlobalModular header of a searched frame: global tree, default weighted-predictor parameters, at most one transform.
void WriteLosslessSearchHeader(BitWriter& bw, int palette_colours, int palette_channels, int rct_type) {
  bw.Bool(true);   // use the global tree
  bw.Bool(true);   // default weighted-predictor parameters
  const bool rct = !palette_colours && rct_type > 0;
  bw.U32(WV(0), WV(1), WB(4, 2), WB(8, 18), palette_colours || rct ? 1 : 0);
  if (palette_colours) {
    bw.Write(2, 1);                                                             // transform id 1: palette
    bw.U32(WB(3), WB(6, 8), WB(10, 72), WB(13, 1096), 0);                       // first channel
    bw.U32(WV(1), WV(3), WV(4), WB(13, 1), (uint32_t)palette_channels);         // channels: colour and alpha together
    bw.U32(WB(8), WB(10, 256), WB(12, 1280), WB(16, 5376), (uint32_t)palette_colours);
    bw.U32(WV(0), WB(8, 1), WB(10, 257), WB(16, 1281), 0);                      // no delta entries
    bw.Write(4, 0);                                                             // (their predictor)
  } else if (rct) {
    bw.Write(2, 0);                                                             // transform id 0: reversible colour transform
    bw.U32(WB(3), WB(6, 8), WB(10, 72), WB(13, 1096), 0);
    bw.U32(WV(6), WB(2), WB(4, 2), WB(6, 10), (uint32_t)rct_type);
  }
}

namespace {

thread_local JxlHipLosslessInfo g_last_lossless;

constexpr int kLlMaxClusters = 12;   // of the effort-9 code: what enc_ll_sections_kernel stages in LDS

// The searched stream(s).  `im` arrives from BeginImage; `fixed` is the stream of effort 7 (the fallback).  Returns the stream to write.
std::vector<uint8_t> CodeLosslessSearched(EncImage& im, const EncSource& src, Arena& A, const EncoderImageMetadata* md, int tier, hipStream_t s, ProgressProc progress,
                                          StageMarks& marks, const std::vector<uint8_t>& fixed, JxlHipLosslessInfo& info) {
  const size_t npx = (size_t)im.w * im.h;
  const bool single = im.ng == 1;
  const int nch_all = (im.gray ? 1 : 3) + im.has_alpha;
  LlSearch ls;
  memset(&ls, 0, sizeof(ls));
  // ---- 1. palette: the distinct pixels over the coded channels.  A palette of one channel would only rename its values.
  std::vector<uint32_t> colours;   // sorted keys
  if (nch_all >= 2) {
    ls.pal_set = A.Get<unsigned long long>(kPalSlots, true);
    ls.pal_count = A.Get<uint32_t>(2, true);
    { const size_t k = marks.Begin("lossless: colour count", s); LaunchEncLosslessSearch(im, ls, 0, s); marks.End(k, s); }
    uint32_t cnt[2];
    ENC_HIP(hipMemcpy(cnt, ls.pal_count, sizeof(cnt), hipMemcpyDeviceToHost));
    if (!cnt[1] && cnt[0] <= kPalCap) {
      std::vector<unsigned long long> set(kPalSlots);
      ENC_HIP(hipMemcpy(set.data(), ls.pal_set, set.size() * 8, hipMemcpyDeviceToHost));
      for (auto v : set) if (v) colours.push_back((uint32_t)v);
      // a fixed order, so that the stream does not depend on which thread inserted first: luma, then alpha, then the key itself
      const bool gray = im.gray, alpha = im.has_alpha;
      auto rank = [gray, alpha](uint32_t k) {
        const uint32_t luma = gray ? (k & 255) * 1000 : 299 * (k & 255) + 587 * ((k >> 8) & 255) + 114 * ((k >> 16) & 255);
        const uint32_t a = alpha ? (k >> (gray ? 8 : 24)) & 255 : 0;
        return ((uint64_t)luma << 40) | ((uint64_t)a << 32) | k;
      };
      std::sort(colours.begin(), colours.end(), [&](uint32_t x, uint32_t y) { return rank(x) < rank(y); });
      std::vector<uint16_t> index(kPalSlots, 0);
      for (size_t slot = 0; slot < set.size(); slot++)
        if (set[slot]) index[slot] = (uint16_t)(std::lower_bound(colours.begin(), colours.end(), (uint32_t)set[slot], [&](uint32_t x, uint32_t y) { return rank(x) < rank(y); }) - colours.begin());
      ls.pal_index = A.Upload(index);
    }
  }
  const int ncol = (int)colours.size();
  Progress(progress, 17);
  // ---- 2. planes and the search over transforms and predictors
  for (int c = 0; c < 4; c++) if (!im.ll_plane[c] && c < nch_all) im.ll_plane[c] = A.Get<int32_t>(npx);
  ls.hist_search = A.Get<uint32_t>((size_t)kLlSlots * kLlPreds * kEncSyms, true);
  im.ll_nch = ncol ? 1 : nch_all;
  im.ll_rct = 0;
  im.ll_tok_extra = 0;
  int slot_of[4] = {0, 1, 2, 3};
  int rct_type = -1;
  {
    const size_t k = marks.Begin("lossless: transform and predictor search", s);
    if (ncol) LaunchEncLosslessSearch(im, ls, 1, s);
    else if (im.gray) LaunchEncLosslessSearch(im, ls, 3, s);
    ls.from_planes = ncol || im.gray;
    LaunchEncLosslessSearch(im, ls, 2, s);
    marks.End(k, s);
  }
  std::vector<uint32_t> hs((size_t)kLlSlots * kLlPreds * kEncSyms);
  ENC_HIP(hipMemcpy(hs.data(), ls.hist_search, hs.size() * 4, hipMemcpyDeviceToHost));
  auto cost = [&](int slot, int pred) { return TokenCost(hs.data() + (size_t)(slot * kLlPreds + pred - 1) * kEncSyms); };
  if (!ls.from_planes) {
    // candidate planes (enc_types.h: kLlSlots) of types 0..6, priced under the gradient predictor; ties go to YCoCg-R
    static const int kSlots[7][3] = {{0, 1, 4}, {0, 1, 5}, {0, 2, 4}, {0, 2, 5}, {0, 3, 4}, {0, 3, 5}, {6, 7, 8}};
    auto type_cost = [&](int t) { return cost(kSlots[t][0], 5) + cost(kSlots[t][1], 5) + cost(kSlots[t][2], 5); };
    rct_type = 6;
    double best = type_cost(6);
    for (int t = 0; t < 6; t++) { const double v = type_cost(t); if (v < best) { best = v; rct_type = t; } }
    for (int c = 0; c < 3; c++) slot_of[c] = kSlots[rct_type][c];
    slot_of[3] = kLlSlots - 1;
    ls.rct_type = rct_type;
    const size_t k = marks.Begin("lossless: planes", s);
    LaunchEncLosslessSearch(im, ls, 3, s);
    marks.End(k, s);
  }
  int32_t pred[5] = {5, 5, 5, 5, 5};   // per coded channel; [ll_nch]: the palette's colours
  double pred_cost[4] = {0, 0, 0, 0};
  for (int c = 0; c < im.ll_nch; c++) {
    pred_cost[c] = cost(slot_of[c], 5);   // ties go to the gradient predictor
    for (int p = 1; p <= 4; p++) { const double v = cost(slot_of[c], p); if (v < pred_cost[c]) { pred_cost[c] = v; pred[c] = p; } }
  }
  Progress(progress, 19);
  // ---- 3. the palette's colours as the host codes them: a channel ncol wide, one row per coded channel
  std::vector<EncToken> pal_tok;
  if (ncol) {
    std::vector<int32_t> meta((size_t)ncol * nch_all);
    for (int c = 0; c < nch_all; c++)
      for (int i = 0; i < ncol; i++) meta[(size_t)c * ncol + i] = (int32_t)((colours[i] >> (8 * c)) & 255);
    auto residuals = [&](int p, std::vector<uint32_t>* out) {
      out->clear();
      for (int y = 0; y < nch_all; y++)
        for (int x = 0; x < ncol; x++) {
          const ModularWNNW hd = ModularWNNWAt([&](int sx, int sy) { return meta[(size_t)sy * ncol + sx]; }, x, y);
          out->push_back(PackSigned(meta[(size_t)y * ncol + x] - ModularPredictWNNW(p, hd.W, hd.N, hd.NW)));
        }
    };
    std::vector<uint32_t> res, best_res;
    double best = 0;
    for (int p : {5, 1, 2, 3, 4}) {
      residuals(p, &res);
      uint32_t h[kEncSyms] = {0};
      for (uint32_t v : res) { uint32_t tok, nb, bits; HybridEncode(v, &tok, &nb, &bits); h[tok]++; }
      const double v = TokenCost(h);
      if (best_res.empty() || v < best) { best = v; best_res = res; pred[1] = p; }
    }
    for (uint32_t v : best_res) pal_tok.push_back(EncToken{0, v});   // (context: below)
  }
  im.tok_ll = im.tok_ll ? im.tok_ll : A.Get<DevToken>((size_t)im.ng * kLlTokCap);
  ls.hist_ll = A.Get<uint32_t>((size_t)kLlMaxLeaves * kEncSyms);
  // One candidate stream: tokens under `use_pred` (and, with wp_ctx, property-15 contexts), code, sections.
  struct Candidate { std::vector<uint8_t> bytes; int32_t pred[4]; int leaves = 0, clusters = 0; };
  auto code = [&](const int32_t* use_pred, bool wp_ctx) {
    Candidate cand;
    int32_t tree_pred[5];
    for (int c = 0; c < im.ll_nch; c++) cand.pred[c] = tree_pred[c] = use_pred[c];
    for (int c = im.ll_nch; c < 4; c++) cand.pred[c] = 0;
    tree_pred[im.ll_nch] = pred[1];
    int pal_ctx = -1;
    std::vector<EncTreeNode> tree = MakeLosslessSearchTree(im.ll_nch, tree_pred, wp_ctx, ncol ? (single ? 1 : 2) : 0, ls.ctx, &pal_ctx);
    cand.leaves = (int)(tree.size() + 1) / 2;
    for (int c = 0; c < 4; c++) ls.pred[c] = cand.pred[c];
    ls.wp_ctx = wp_ctx;
    im.ll_tok_extra = ncol && single ? (uint32_t)pal_tok.size() : 0;
    ENC_HIP(hipMemset(ls.hist_ll, 0, (size_t)kLlMaxLeaves * kEncSyms * 4));
    { const size_t k = marks.Begin(wp_ctx ? "lossless: tokens (property-15 contexts)" : "lossless: tokens", s); LaunchEncLosslessSearch(im, ls, 5, s); marks.End(k, s); }
    std::vector<uint32_t> hist((size_t)cand.leaves * kEncSyms);
    ENC_HIP(hipMemcpy(hist.data(), ls.hist_ll, hist.size() * 4, hipMemcpyDeviceToHost));
    if (ncol) {
      for (auto& t : pal_tok) {
        t.ctx = (uint32_t)pal_ctx;
        uint32_t tok, nb, bits;
        HybridEncode(t.value, &tok, &nb, &bits);
        hist[(size_t)pal_ctx * kEncSyms + tok]++;
      }
      if (single) {
        std::vector<DevToken> dt;
        for (auto& t : pal_tok) dt.push_back(DevToken{t.ctx, t.value});
        ENC_HIP(hipMemcpy(im.tok_ll, dt.data(), dt.size() * sizeof(DevToken), hipMemcpyHostToDevice));
      }
    }
    BitWriter lf_global;
    EncCode mcode;
    lf_global.Bool(true);   // default LF dequantisation factors
    lf_global.Bool(true);   // global MA tree
    WriteTree(tree, lf_global);
    BuildAndWriteCode(hist.data(), (size_t)cand.leaves, std::min(kLlMaxClusters, cand.leaves), {}, lf_global, mcode);
    cand.clusters = (int)mcode.num_clusters;
    WriteLosslessSearchHeader(lf_global, ncol, nch_all, rct_type);
    if (ncol && !single) WriteTokensHost(pal_tok, mcode, lf_global);   // the colours are the global stream's only channel
    const size_t k = marks.Begin(wp_ctx ? "lossless: sections (property-15 contexts)" : "lossless: sections", s);
    cand.bytes = FinishLossless(im, src, A, mcode, lf_global, md, s);
    marks.End(k, s);
    return cand;
  };
  Candidate chosen = code(pred, false);
  Progress(progress, 22);
  // ---- 4. effort 9: the weighted predictor's state on the encode side.  Palette frames stay as they are.
  if (tier >= 9 && !ncol) {
    for (int c = 0; c < im.ll_nch; c++) { ls.wp_pred[c] = A.Get<int32_t>(npx); ls.wp_prop[c] = A.Get<int32_t>(npx); }
    ls.hist_wp = A.Get<uint32_t>(4 * kEncSyms, true);
    { const size_t k = marks.Begin("lossless: weighted pass", s); LaunchEncLosslessSearch(im, ls, 4, s); marks.End(k, s); }
    std::vector<uint32_t> hw(4 * kEncSyms);
    ENC_HIP(hipMemcpy(hw.data(), ls.hist_wp, hw.size() * 4, hipMemcpyDeviceToHost));
    int32_t pred9[4];
    for (int c = 0; c < im.ll_nch; c++) pred9[c] = TokenCost(hw.data() + (size_t)c * kEncSyms) < pred_cost[c] ? 6 : pred[c];
    Progress(progress, 24);
    Candidate with_ctx = code(pred9, true);
    if (with_ctx.bytes.size() < chosen.bytes.size()) chosen = std::move(with_ctx);
  }
  Progress(progress, 27);
  info.tier = tier;
  info.palette_colours = ncol;
  info.rct_type = rct_type;
  info.num_channels = im.ll_nch;
  for (int c = 0; c < 4; c++) info.predictor[c] = chosen.pred[c];
  info.leaves = chosen.leaves;
  info.clusters = chosen.clusters;
  info.searched_bytes = chosen.bytes.size();
  info.effort7_bytes = fixed.size();
  info.fell_back_to_effort7 = chosen.bytes.size() < fixed.size() ? 0 : 1;   // never larger than effort 7: only a strictly smaller stream is written
  return info.fell_back_to_effort7 ? fixed : chosen.bytes;
}

// Lossless: a Modular frame in the original (sRGB) colour space (Encoder/JxlEncoder.cpp:214,325).  Efforts up to 7 write the fixed
// stream; 8 and 9 also search palette, colour transform, predictors and (9) contexts, and write the smaller of the two.
void EncodeLossless(const EncSource& src, const EncoderOptions* opt, const EncoderImageMetadata* md, IOCallbacks* io, ProgressProc progress) {
  Arena A;
  hipStream_t s = nullptr;
  EncImage im;
  BeginImage(src, md, A, im, progress);
  im.lossless = 1;
  im.ll_nch = (im.gray ? 1 : 3) + im.has_alpha;
  LayLosslessPlanes(A, im);
  Progress(progress, 15);
  // the search keys palettes and candidates on bytes: samples of more than 8 bits get the fixed stream at every effort
  const int tier = src.deep() ? 0 : (opt->effort >= 9 ? 9 : (opt->effort >= 8 ? 8 : 0));
  std::vector<uint8_t> codestream = CodeLosslessFixed(im, src, A, md, s, tier ? nullptr : progress);
  if (tier) {
    StageMarks marks;
    JxlHipLosslessInfo info;
    memset(&info, 0, sizeof(info));
    codestream = CodeLosslessSearched(im, src, A, md, tier, s, progress, marks, codestream, info);
    marks.Publish(&g_last_save_stages);
    g_last_lossless = info;
  }
  Progress(progress, 30);
  EmitFile(codestream, md, io, progress);
}

// What this project's decoder shows of an interim stream of the closed loop, as XYB planes after every loop filter: the stream goes
// through a JxlHipDecoder that keeps its stage copies ("debug_taps"), and the filtered planes (wp x hp, as the decoder lays them out)
// are copied into the encoder's device planes.  Biases, LF smoothing and the EPF sigma of the quant field are the decoder's own.
struct ReconDecoder {
  JxlHipDecoder* dec = nullptr;
  uint8_t* d_out = nullptr;
  std::vector<float> host;
  ReconDecoder(Arena& A, size_t out_bytes) {
    ErrorInfo err;
    memset(&err, 0, sizeof(err));
    dec = jxlhip_decoder_create(-1, &err);
    if (!dec) throw EncFail(EncoderStatus_EncodeError, std::string("closed loop: the decoder could not be created: ") + err.errorMessage);
    (void)jxlhip_set_option(dec, "debug_taps", 1);
    d_out = A.Get<uint8_t>(out_bytes);
  }
  ~ReconDecoder() { jxlhip_decoder_destroy(dec); }
  ReconDecoder(const ReconDecoder&) = delete;
  ReconDecoder& operator=(const ReconDecoder&) = delete;
  void Reconstruct(const std::vector<uint8_t>& cs, float* const* planes, size_t npad) {
    const uint8_t* data = cs.data();
    const uint8_t* dev_data = nullptr;
    const size_t size = cs.size();
    uint8_t* out = d_out;
    DecoderStatus st = DecoderStatus_Ok;
    ErrorInfo err;
    memset(&err, 0, sizeof(err));
    if (jxlhip_decode_batch(dec, 1, &data, &size, &dev_data, &out, nullptr, 1, &st, &err) != DecoderStatus_Ok)
      throw EncFail(EncoderStatus_EncodeError, std::string("closed loop: an interim stream did not decode: ") + err.errorMessage);
    host.resize(npad);
    for (int c = 0; c < 3; c++) {
      if (jxlhip_read_plane(dec, 0, "xyb_filtered", c, host.data(), npad * 4) != npad * 4)
        throw EncFail(EncoderStatus_EncodeError, "closed loop: the decoder's filtered planes have another size than the encoder's");
      ENC_HIP(hipMemcpy(planes[c], host.data(), npad * 4, hipMemcpyHostToDevice));
    }
  }
};

// What the distance and the effort of a lossy save fix before any pixel is looked at
struct LossyParams {
  EncFrameInfo fi;
  uint32_t global_scale, quant_lf;
};
// quantiser and loop-filter parameters (distance, :319); the effort picks the transform set
LossyParams SetLossyParams(const EncoderOptions* opt, EncImage& im) {
  LossyParams qp;
  EncFrameInfo& fi = qp.fi;
  const float distance = std::max(0.05f, std::min(25.0f, opt->distance));
  fi.encoding = 0;
  fi.gab = true;
  fi.epf_iters = 0;
  for (float t : {0.7f, 1.5f, 4.0f}) if (distance >= t) fi.epf_iters++;
  const double qf = 0.85 / distance;
  const uint32_t global_scale = (uint32_t)std::max<long>(1, std::min<long>(8193 + 65535, std::lrint(65536.0 * qf / 16.0)));
  const uint32_t quant_lf = (uint32_t)std::max<long>(1, std::min<long>(65536, std::lrint(1.1 / distance * 65536.0 / global_scale)));
  const float inv_gs = 65536.0f / global_scale;
  const float m_lf[3] = {1.0f / 4096, 1.0f / 512, 1.0f / 256};
  for (int c = 0; c < 3; c++) im.inv_mul_lf[c] = 1.0f / (m_lf[c] * inv_gs / quant_lf);
  im.mul_lf_y = m_lf[1] * inv_gs / quant_lf;
  im.inv_gs = inv_gs;
  im.x_dm = std::pow(0.8f, (float)fi.x_qm_scale - 2.0f);
  im.b_dm = std::pow(0.8f, (float)fi.b_qm_scale - 2.0f);
  im.qbias1 = 1.0f - 0.07005449891748593f;
  im.qbias3 = 0.145f;
  im.gab = fi.gab;
  {
    const float w1 = 0.115169525f, w2 = 0.061248592f, div = 1.0f + 4.0f * (w1 + w2);
    for (int c = 0; c < 3; c++) { im.gab_w[c][0] = 1.0f / div; im.gab_w[c][1] = w1 / div; im.gab_w[c][2] = w2 / div; }
  }
  // effort (JxlEncoderTypes.h:29, passed to the encoder library as its effort setting, Encoder/JxlEncoder.cpp:319-326): the library's
  // fast settings (1..4) keep every block an 8x8 DCT; 5 and 6 add 16x16 / 32x32 DCTs on flat regions; from 7 (the host's default) the
  // 64x64 and the rectangular 16x8 ... 64x32 shapes join; 8 and 9 keep that set and correct the quant field in a closed loop (below)
  im.squares = opt->effort >= 7 ? 2 : (opt->effort >= 5 ? 1 : 0);
  qp.global_scale = global_scale; qp.quant_lf = quant_lf;
  return qp;
}

// The tables the front end reads (see EncImage), uploaded through `A`
void UploadEncTables(Arena& A, EncImage& im) {
  const StaticTables& st = GetStaticTables();
  {
    for (auto& q : im.scan_of) q = nullptr;
    for (auto& q : im.dq) q = nullptr;
    for (int o : {0, 2, 3, 4, 6, 7, 8}) {   // order buckets of DCT8, 16x16, 32x32, 16x8 / 8x16, 32x16 / 16x32, 64x64, 64x32 / 32x64
      const std::vector<uint16_t>& order = st.natural_order[o];   // scan position -> stored index
      std::vector<uint16_t> inv(order.size());
      for (size_t k = 0; k < order.size(); k++) inv[order[k]] = (uint16_t)k;
      im.scan_of[o] = A.Upload(inv);
    }
    for (int q : {0, 4, 5, 6, 8, 11, 12}) im.dq[q] = A.Upload(st.dq[q]);
    std::vector<float> rs(16 * 64, 1.0f);
    for (int l = 0; l < 4; l++) {
      const int N = 8 << l, c = 1 << l;
      im.basis[l] = A.Upload(st.basis[l]);
      std::vector<float> div(st.basis[l]);
      for (auto& v : div) v = v / (float)N;
      im.basis_div[l] = A.Upload(div);
      std::vector<float> small((size_t)c * c);
      for (int k = 0; k < c; k++)
        for (int n = 0; n < c; n++) small[(size_t)k * c + n] = (float)((k ? std::sqrt(2.0) : 1.0) * std::cos((2 * n + 1) * k * M_PI / (2.0 * c)));
      im.bsmall[l] = A.Upload(small);
    }
    auto resample = [](int c, int k) {   // coefficient k of an 8c-point DCT from the c-point DCT of the block means
      if (k == 0) return 1.0;
      const double t = k * M_PI / (2.0 * c);
      return 1.0 / (std::cos(t / 2) * std::cos(t / 4) * std::cos(t / 8));
    };
    for (int ly = 0; ly < 4; ly++)
      for (int lx = 0; lx < 4; lx++)
        for (int ky = 0; ky < (1 << ly); ky++)
          for (int kx = 0; kx < (1 << lx); kx++) rs[(ly * 4 + lx) * 64 + ky * 8 + kx] = (float)(resample(1 << ly, ky) * resample(1 << lx, kx));
    im.rs = A.Upload(rs);
  }
}

// the same tables for another image: they depend on nothing of it
void CopyEncTables(const EncImage& from, EncImage& to) {
  memcpy(to.scan_of, from.scan_of, sizeof(to.scan_of));
  memcpy(to.dq, from.dq, sizeof(to.dq));
  memcpy(to.basis, from.basis, sizeof(to.basis));
  memcpy(to.basis_div, from.basis_div, sizeof(to.basis_div));
  memcpy(to.bsmall, from.bsmall, sizeof(to.bsmall));
  to.rs = from.rs;
}

// LfGlobal of a lossy frame up to and including the Modular code: quantiser, MA tree, the code of the Modular streams' token
// histograms hist_mod[kNumEncLeaves][kEncSyms], and the global Modular image header of a frame with alpha.
void WriteLossyLfGlobal(const EncImage& im, const LossyParams& qp, const uint32_t* hist_mod, BitWriter& lf_global, EncCode& mcode) {
  lf_global.Bool(true);   // default LF dequantisation factors
  lf_global.U32(WB(11, 1), WB(11, 2049), WB(12, 4097), WB(16, 8193), qp.global_scale);
  lf_global.U32(WV(16), WB(5, 1), WB(8, 1), WB(16, 1), qp.quant_lf);
  lf_global.Bool(true);   // default block-context map
  lf_global.Bool(true);   // default LF chroma-from-luma parameters
  lf_global.Bool(true);   // global MA tree
  // fitted chroma-from-luma maps wrote tokens unless every value of the frame is 0 (enc_meta_tokens_kernel); the frame is then the
  // one without fitting
  bool cfl_maps = false;
  for (uint32_t k = 0; k < kEncSyms; k++) cfl_maps |= hist_mod[kLeafCfl * kEncSyms + k] != 0;
  WriteTree(MakeEncoderTree((uint32_t)im.nlf, cfl_maps), lf_global);
  {
    std::vector<uint8_t> pinned(kNumEncLeaves, 0);
    pinned[kLeafSharp] = 1;                      // constant channels: no token is ever written
    pinned[kLeafCfl] = cfl_maps ? 0 : 1;
    pinned[kLeafStrategy] = im.squares ? 0 : 1;  // ... and so is the strategy row while every block is an 8x8 DCT
    BuildAndWriteCode(hist_mod, kNumEncLeaves, kEncModClusters, pinned, lf_global, mcode);
  }
  if (im.has_alpha) lf_global.Write(4, 3);   // global Modular image header: global tree, default predictor, no transforms
}

// HfGlobal: default matrices, one preset, natural orders, the code of the HF token histograms hist_ac[kAcContexts][kEncSyms]
void WriteLossyHfGlobal(const EncImage& im, const uint32_t* hist_ac, BitWriter& hf_global, EncCode& acode) {
  hf_global.Bool(true);                      // default dequantisation matrices
  hf_global.Write(im.ng <= 1 ? 0 : 32 - __builtin_clz((unsigned)(im.ng - 1)), 0);   // one HF preset
  hf_global.U32(WV(0x5F), WV(0x13), WV(0), WB(kNumOrders), 0);                       // natural coefficient orders
  BuildAndWriteCode(hist_ac, kAcContexts, kEncHfClusters, {}, hf_global, acode);
}

// The codestream of a lossy frame from its finished LfGlobal and HfGlobal and the coded sections: packed + off[s], sec_bits[s] for
// section s (LF groups, groups, then the global alpha stream of a one-group frame).  frame_only: a frame of an animation (ii: its
// canvas, fi.at: where it lies), without the image header.
std::vector<uint8_t> AssembleLossy(const EncImage& im, const EncImageInfo& ii, const EncFrameInfo& fi, BitWriter& lf_global, BitWriter& hf_global,
                                   const uint8_t* packed, const uint64_t* off, const uint64_t* sec_bits, bool frame_only = false) {
  BitWriter cs;
  if (!frame_only) WriteCodestreamHeaders(ii, cs);
  WriteFrameHeader(ii, fi, cs);
  auto bytes = [&](int sec) { return std::vector<uint8_t>(packed + off[sec], packed + off[sec] + ((sec_bits[sec] + 7) >> 3)); };
  std::vector<std::vector<uint8_t>> sections;
  if (im.ng == 1) {
    // LfGlobal | LfGroup | HfGlobal | PassGroup share one bit stream
    if (im.has_alpha) lf_global.AppendBits(packed + off[im.nlf + im.ng], sec_bits[im.nlf + im.ng]);
    const uint64_t hg_bits = hf_global.BitCount();
    std::vector<uint8_t> hg = hf_global.Finish();
    lf_global.AppendBits(packed + off[0], sec_bits[0]);
    lf_global.AppendBits(hg.data(), hg_bits);
    lf_global.AppendBits(packed + off[1], sec_bits[1]);
    sections.push_back(lf_global.Finish());
  } else {
    sections.push_back(lf_global.Finish());
    for (int g = 0; g < im.nlf; g++) sections.push_back(bytes(g));
    sections.push_back(hf_global.Finish());
    for (int g = 0; g < im.ng; g++) sections.push_back(bytes(im.nlf + g));
  }
  std::vector<uint32_t> sizes;
  for (auto& sec : sections) sizes.push_back((uint32_t)sec.size());
  WriteToc(sizes, cs);
  std::vector<uint8_t> out = cs.Finish();
  for (auto& sec : sections) out.insert(out.end(), sec.begin(), sec.end());
  return out;
}

void EncodeLossy(const EncSource& src, const EncoderOptions* opt, const JxlHipLossyOptions& lossy, const EncoderImageMetadata* md, IOCallbacks* io,
                 ProgressProc progress) {
  Arena A;
  hipStream_t s = nullptr;
  EncImage im;
  PhaseClock clk;
  BeginImage(src, md, A, im, progress);
  if (md->iccProfile && md->iccProfileSize) {
    // Lossy with a profile: the samples reach XYB through the profile (the reference leaves that to its encoder library's colour
    // management, Encoder/JxlEncoder.cpp:258-268).  Matrix / TRC profiles are evaluated here; a profile that would need a full
    // colour management system cannot be encoded lossily without misrepresenting its colours.
    IccModel model;
    if (!IccBuildModel(md->iccProfile, md->iccProfileSize, &model) || model.gray)
      throw EncFail(EncoderStatus_EncodeError, "this ICC profile is not an RGB matrix/TRC profile: lossy saving needs a full colour management system (save lossless instead)");
    std::vector<float> lin;
    for (int c = 0; c < 3; c++) lin.insert(lin.end(), model.to_linear[c].begin(), model.to_linear[c].end());
    float* d_lin = A.Get<float>(lin.size());
    ENC_HIP(hipMemcpy(d_lin, lin.data(), lin.size() * 4, hipMemcpyHostToDevice));
    im.icc_lin = d_lin;
    for (int k = 0; k < 9; k++) im.icc_to_srgb[k] = (float)model.to_linear_srgb[k];
  }
  clk.Lap("upload + analysis");
  const uint32_t w = src.width(), h = src.height();
  const size_t npx = (size_t)w * h, npad = (size_t)im.wp * im.hp, ncell = (size_t)im.w8 * im.h8;
  // ---- 2. quantiser and loop-filter parameters, transform set, tables
  const LossyParams qp = SetLossyParams(opt, im);
  const EncFrameInfo& fi = qp.fi;
  UploadEncTables(A, im);
  // ---- 3. planes, front end
  im.cfl = lossy.chroma_from_luma;
  LayLossyPlanes(A, im);
  Progress(progress, 15);
  clk.Lap("allocation");
  StageMarks marks;
  { const size_t k = marks.Begin("front_end (xyb, sharpen, activity, strategy, DCT + quantise)", s); LaunchEncFrontEnd(im, s); marks.End(k, s); }
  clk.Lap("xyb + sharpen + dct/quant");
  Progress(progress, 20);
  // ---- 4. .. 7. are CodeField below: everything that follows from the quantised data.  Efforts up to 7 run it once; the closed loop
  // of efforts 8 and 9 runs it once per evaluation.  Its buffers are allocated here, its counters cleared at every run.
  LayLossyCoding(A, im);
  const int nsec = EncNumSections(im);   // + the global alpha stream of single-group frames
  // The Modular streams' recurrences run on a stream of their own (the LF coefficients of an LF group are the longest of the frame),
  // the HF streams' beside them.
  hipStream_t s_ans = nullptr, s_hf = nullptr;
  ENC_HIP(hipStreamCreateWithFlags(&s_ans, hipStreamNonBlocking));
  struct StreamGuard { hipStream_t s; ~StreamGuard() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } } } s_ans_guard{s_ans};
  ENC_HIP(hipStreamCreateWithFlags(&s_hf, hipStreamNonBlocking));
  StreamGuard s_hf_guard{s_hf};
  const EncImageInfo ii = DescribeImage(im, src, md, true);
  // The codestream of the quantised data in `im`.  `final`: the call whose stream is (normally) written: it reports progress 25 and
  // 30; `mk`: where its kernel groups are timed (null: nowhere).
  auto CodeField = [&](bool final, StageMarks* mk, bool publish) -> std::vector<uint8_t> {
    Arena E;   // the codes of this run
    auto begin = [&](const char* name, hipStream_t st) { return mk ? mk->Begin(name, st) : (size_t)-1; };
    auto end = [&](size_t k, hipStream_t st) { if (mk) mk->End(k, st); };
    ENC_HIP(hipMemset(im.n_ac, 0, std::max<size_t>((size_t)im.ng * 4, 256)));
    ENC_HIP(hipMemset(im.n_meta, 0, std::max<size_t>((size_t)im.nlf * 4, 256)));
    ENC_HIP(hipMemset(im.hist_mod, 0, kNumEncLeaves * kEncSyms * 4));
    ENC_HIP(hipMemset(im.hist_ac, 0, (size_t)kAcContexts * kEncSyms * 4));
    ENC_HIP(hipMemset(im.sec_bits, 0, std::max<size_t>((size_t)nsec * 8, 256)));
    ENC_HIP(hipMemset(im.stream_state, 0, std::max<size_t>(EncNumStreamStates(im) * 4, 256)));
    // ---- 4. tokens + histograms
    { const size_t k = begin("tokens + histograms", s); LaunchEncTokens(im, s); end(k, s); }
    std::vector<uint32_t> hist_mod(kNumEncLeaves * kEncSyms), hist_ac((size_t)kAcContexts * kEncSyms);
    ENC_HIP(hipMemcpy(hist_mod.data(), im.hist_mod, hist_mod.size() * 4, hipMemcpyDeviceToHost));
    ENC_HIP(hipMemcpy(hist_ac.data(), im.hist_ac, hist_ac.size() * 4, hipMemcpyDeviceToHost));
    clk.Lap("tokens + histograms");
    if (final) Progress(progress, 25);
    // ---- 5. LfGlobal and HfGlobal (host): quantiser, MA tree, entropy codes
    BitWriter lf_global, hf_global;
    EncCode mcode, acode;
    WriteLossyLfGlobal(im, qp, hist_mod.data(), lf_global, mcode);
    clk.Lap("host: tree + modular code");
    // The Modular code is ready: start the recurrences of its streams on their stream, and build the HF code meanwhile.
    im.mcode = UploadCode(E, mcode);
    ENC_HIP(hipDeviceSynchronize());   // tokens, histogram downloads and the clears above are done before the other stream starts
    { const size_t k = begin("ans recurrences, Modular streams (LF, metadata, alpha)", s_ans); LaunchEncReverse(im, 0, s_ans); end(k, s_ans); }
    {
      const auto t0 = std::chrono::steady_clock::now();
      WriteLossyHfGlobal(im, hist_ac.data(), hf_global, acode);
      if (clk.on) fprintf(stderr, "[enc] %-28s %8.2f ms (host only)\n", "HF code construction", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    clk.Lap("host: HF code (overlaps the LF recurrences)");
    // ---- 6. ANS coding of every section on the GPU (the Modular streams' recurrences have been running since their code was built)
    im.acode = UploadCode(E, acode);
    { const size_t k = begin("ans recurrences, HF streams", s_hf); LaunchEncReverse(im, 1, s_hf); end(k, s_hf); }
    {
      hipEvent_t hf_done;
      ENC_HIP(hipEventCreateWithFlags(&hf_done, hipEventDisableTiming));
      ENC_HIP(hipEventRecord(hf_done, s_hf));
      ENC_HIP(hipStreamWaitEvent(s_ans, hf_done, 0));
      const size_t k = begin("section bit layout", s_ans);
      LaunchEncSections(im, s_ans);   // bit layout of every section: needs the states of both kinds of stream
      end(k, s_ans);
      ENC_HIP(hipStreamSynchronize(s_ans));
      (void)hipEventDestroy(hf_done);
    }
    clk.Lap("ans sections");
    std::vector<uint64_t> sec_bits(nsec);
    ENC_HIP(hipMemcpy(sec_bits.data(), im.sec_bits, sec_bits.size() * 8, hipMemcpyDeviceToHost));
    std::vector<uint64_t> off(nsec + 1, 0);
    for (int i = 0; i < nsec; i++) off[i + 1] = off[i] + ((sec_bits[i] + 7) >> 3);
    std::vector<uint8_t> packed(std::max<uint64_t>(off[nsec], 1));
    {
      uint64_t* d_off = E.Upload(off);
      uint8_t* d_packed = E.Get<uint8_t>(packed.size());
      const size_t k = begin("compact", s);
      LaunchEncCompact(im, d_off, d_packed, nsec, s);
      end(k, s);
      ENC_HIP(hipMemcpy(packed.data(), d_packed, packed.size(), hipMemcpyDeviceToHost));
    }
    ENC_HIP(hipGetLastError());
    if (mk && publish) mk->Publish(&g_last_save_stages);
    clk.Lap("compact + download");
    if (final) Progress(progress, 30);
    // ---- 7. codestream assembly
    return AssembleLossy(im, ii, fi, lf_global, hf_global, packed.data(), off.data(), sec_bits.data());
  };
  std::vector<uint8_t> codestream;
  const int corrections = opt->effort >= 9 ? 4 : (opt->effort >= 8 ? 2 : 0);
  if (!corrections) {
    codestream = CodeField(true, &marks, true);
  } else {
    // ---- closed loop ("Distance map" and "The loop of efforts 8 and 9"): code the field, reconstruct what a decoder
    // shows, measure, correct the field, again.  The strategies stay; only the quant field moves, so every interim stream is valid.
    static const char* const kEvalName[5] = {"evaluation 0 (code, decode, distance map)", "evaluation 1 (code, decode, distance map)",
                                             "evaluation 2 (code, decode, distance map)", "evaluation 3 (code, decode, distance map)",
                                             "evaluation 4 (code, decode, distance map)"};
    int32_t* q0 = A.Get<int32_t>(ncell);
    ENC_HIP(hipMemcpy(q0, im.rawq, ncell * 4, hipMemcpyDeviceToDevice));
    DistMap dm = MakeDistMap(im.w, im.h);
    float* recon[3];
    for (int c = 0; c < 3; c++) { dm.orig[c] = im.xyb[c]; recon[c] = A.Get<float>(npad); dm.recon[c] = recon[c]; }
    dm.recon_stride = im.wp;
    dm.mask = A.Get<float>(npx);
    dm.cell = A.Get<float>(ncell);
    LaunchDistMask(dm, s);
    ReconDecoder rd(A, (size_t)w * h * 4 * src.sample_bytes());   // what the decoder writes: up to four samples per pixel
    std::vector<float> cells(ncell), cells0, sorted;
    float tau = 0.f;
    int over_first = 0, over_last = 0;
    const int nev = corrections + 1;
    for (int e = 0; e < nev; e++) {
      const size_t k = marks.Begin(kEvalName[e], s);
      if (e) LaunchEncVarblocks(im, s);
      codestream = CodeField(e == nev - 1, e == nev - 1 ? &marks : nullptr, false);
      rd.Reconstruct(codestream, recon, npad);
      LaunchDistCells(dm, s);
      ENC_HIP(hipMemcpy(cells.data(), dm.cell, ncell * 4, hipMemcpyDeviceToHost));
      marks.End(k, s);
      if (e == 0) {
        sorted = cells;
        std::sort(sorted.begin(), sorted.end());
        tau = sorted[(size_t)std::floor(0.9 * (double)(ncell - 1))];   // the 90th percentile, rank rounded down
        cells0 = cells;
      }
      int over = 0;
      for (float t : cells) over += t > tau;
      if (e == 0) over_first = over;
      over_last = over;
      if (e < nev - 1) {
        LaunchDistCorrect(im, dm.cell, q0, tau, kLoopPUp, kLoopPDown, e < nev - 2, s);
        Progress(progress, 20);   // the loop's value until its last evaluation: a cancel lands within one evaluation
      }
    }
    if (over_last > over_first) {   // never worse than effort 7 by this count: its field is written instead
      ENC_HIP(hipMemcpy(im.rawq, q0, ncell * 4, hipMemcpyDeviceToDevice));
      LaunchEncVarblocks(im, s);
      codestream = CodeField(false, nullptr, false);
      cells = cells0;
      over_last = over_first;
    }
    ENC_HIP(hipGetLastError());
    marks.Publish(&g_last_save_stages);
    g_last_dist.cells = cells;
    g_last_dist.evaluations = nev;
    g_last_dist.target = tau;
    g_last_dist.over_first = over_first;
    g_last_dist.over_emitted = over_last;
  }
  clk.Lap("assembly");
  EmitFile(codestream, md, io, progress);
  clk.Lap("container + write callbacks");
}

}  // namespace
}  // namespace jxlhip

using namespace jxlhip;

// Device time of the kernel groups of this thread's last lossy SaveImage (see StageMarks)
extern "C" JXLFILETYPEIO_API int32_t jxlhip_last_save_stage_times(const char** names, float* ms, int32_t capacity) {
  int32_t k = 0;
  for (auto& e : g_last_save_stages) {
    if (k >= capacity) break;
    if (names) names[k] = e.first;
    if (ms) ms[k] = e.second;
    k++;
  }
  return k;
}

// The closed loop's figures of this thread's last SaveImage (evaluations == 0: an effort below 8 or a lossless save; no cells)
extern "C" JXLFILETYPEIO_API size_t jxlhip_last_save_distances(float* dst, size_t capacity, int32_t* evaluations, float* target,
                                                               int32_t* cells_over_target_first, int32_t* cells_over_target_emitted) {
  const LastDistances& d = g_last_dist;
  if (dst) memcpy(dst, d.cells.data(), std::min(capacity, d.cells.size()) * sizeof(float));
  if (evaluations) *evaluations = d.evaluations;
  if (target) *target = d.target;
  if (cells_over_target_first) *cells_over_target_first = d.over_first;
  if (cells_over_target_emitted) *cells_over_target_emitted = d.over_emitted;
  return d.cells.size();
}

// What the search of this thread's last lossless SaveImage at effort 8 or 9 chose (tier 0: any other save)
extern "C" JXLFILETYPEIO_API void jxlhip_last_save_lossless_info(JxlHipLosslessInfo* out) {
  if (out) *out = g_last_lossless;
}

// The distance map of picture b against the original a (both BGRA8 in host memory, alpha ignored), through the encoder's
// sRGB -> XYB conversion: ceil(w / 8) * ceil(h / 8) cell distances, rows of cells top to bottom.
extern "C" JXLFILETYPEIO_API EncoderStatus jxlhip_distance_map(const uint8_t* a_bgra, uint32_t stride_a, const uint8_t* b_bgra, uint32_t stride_b,
                                                               uint32_t w, uint32_t h, float* cell_dist, size_t capacity, ErrorInfo* err) {
  if (!a_bgra || !b_bgra || !cell_dist) return EncoderStatus_NullParameter;
  try {
    if (!w || !h || w > (1u << 30) / h || stride_a < (uint64_t)w * 4 || stride_b < (uint64_t)w * 4)
      throw EncFail(EncoderStatus_EncodeError, "invalid bitmap");
    DistMap dm = MakeDistMap((int32_t)w, (int32_t)h);
    const size_t npx = (size_t)w * h, ncell = (size_t)dm.w8 * dm.h8;
    if (capacity < ncell) throw EncFail(EncoderStatus_EncodeError, "the buffer for the cell distances is too small");
    Arena A;
    float* planes[2][3];
    for (int k = 0; k < 2; k++) {
      const uint8_t* src = k ? b_bgra : a_bgra;
      const uint32_t stride = k ? stride_b : stride_a;
      EncImage im;
      memset(&im, 0, sizeof(im));
      im.w = (int32_t)w; im.h = (int32_t)h; im.stride = (int64_t)stride;
      im.transfer = kTransferSrgb;
      uint8_t* d_bgra = A.Get<uint8_t>((size_t)stride * h);
      ENC_HIP(hipMemcpy(d_bgra, src, (size_t)stride * (h - 1) + (size_t)w * 4, hipMemcpyHostToDevice));   // the last row may end at its pixels
      im.bgra = d_bgra;
      for (int c = 0; c < 3; c++) planes[k][c] = im.xyb[c] = A.Get<float>(npx);
      LaunchEncXyb(im, nullptr);
    }
    for (int c = 0; c < 3; c++) { dm.orig[c] = planes[0][c]; dm.recon[c] = planes[1][c]; }
    dm.recon_stride = (int32_t)w;
    dm.mask = A.Get<float>(npx);
    dm.cell = A.Get<float>(ncell);
    LaunchDistMask(dm, nullptr);
    LaunchDistCells(dm, nullptr);
    ENC_HIP(hipMemcpy(cell_dist, dm.cell, ncell * 4, hipMemcpyDeviceToHost));
    ENC_HIP(hipGetLastError());
    return EncoderStatus_Ok;
  } catch (const EncFail& e) {
    if (e.status == EncoderStatus_EncodeError) SetEncErr(err, e.what());
    return e.status;
  } catch (const std::exception& e) {
    SetEncErr(err, e.what());
    return EncoderStatus_EncodeError;
  } catch (...) {
    return EncoderStatus_EncodeError;
  }
}

extern "C" JXLFILETYPEIO_API EncoderStatus SaveImage(const BitmapData* bitmap, const EncoderOptions* options, const EncoderImageMetadata* metadata,
                                   IOCallbacks* callbacks, ErrorInfo* err, ProgressProc progress) {
  if (!bitmap || !options || !callbacks || !metadata) return EncoderStatus_NullParameter;   // Encoder/JxlEncoder.cpp:155-158
  try {
    g_last_dist = LastDistances();
    g_last_lossless = JxlHipLosslessInfo();
    Progress(progress, 0);   // :162
    if (!callbacks->Write) throw EncFail(EncoderStatus_NullParameter, "");
    EncSource src;
    src.bmp = bitmap;
    if (options->lossless) EncodeLossless(src, options, metadata, callbacks, progress);   // :214,325
    else EncodeLossy(src, options, JxlHipLossyOptions{}, metadata, callbacks, progress);
    return EncoderStatus_Ok;
  } catch (const EncFail& e) {
    if (e.status == EncoderStatus_EncodeError) SetEncErr(err, e.what());
    return e.status;
  } catch (const std::bad_alloc&) {
    return EncoderStatus_OutOfMemory;
  } catch (const std::exception& e) {
    SetEncErr(err, e.what());
    return EncoderStatus_EncodeError;
  } catch (...) {
    return EncoderStatus_EncodeError;   // never throw across the ABI (:382-389)
  }
}

namespace {

// The refusals of jxlhip_save_pixels, decided on the host before any HIP call.  Fills `src` with what the headers will say.
void CheckPixels(const JxlHipPixels* px, const EncoderOptions* opt, const EncoderImageMetadata* md, EncSource& src) {
  auto refuse = [](const char* why) { throw EncFail(EncoderStatus_EncodeError, why); };
  if (!px->data) throw EncFail(EncoderStatus_NullParameter, "");
  if (!px->width || !px->height) refuse("the image has no pixels");
  if (px->width > (1u << 30) / px->height) refuse("the image is too large");
  if (px->num_channels < 1 || px->num_channels > 4) refuse("the number of channels must be 1 (Gray), 2 (Gray, A), 3 (R, G, B) or 4 (R, G, B, A)");
  size_t sample_bytes = 0;
  switch (px->sample_type) {
    case ImageChannelRepresentation_Uint8:
      if (px->bits_per_sample != 8) refuse("bits_per_sample must be 8 for Uint8 samples");
      src.bits = 8; sample_bytes = 1;
      break;
    case ImageChannelRepresentation_Uint16:
      if (px->bits_per_sample < 9 || px->bits_per_sample > 16) refuse("bits_per_sample must be 9..16 for Uint16 samples");
      src.bits = (uint32_t)px->bits_per_sample; sample_bytes = 2;
      break;
    case ImageChannelRepresentation_Float16:
    case ImageChannelRepresentation_Float32:
      if (px->bits_per_sample != 0) refuse("bits_per_sample must be 0 for float samples");
      if (px->sample_type == ImageChannelRepresentation_Float16) { src.bits = 16; src.exp_bits = 5; sample_bytes = 2; }
      else { src.bits = 32; src.exp_bits = 8; sample_bytes = 4; }
      break;
    default: refuse("unknown sample type");
  }
  if (px->stride_bytes < (uint64_t)px->width * (uint64_t)px->num_channels * sample_bytes) refuse("stride_bytes is smaller than a row of pixels");
  const bool gray = px->num_channels < 3;
  switch (px->colour) {
    case KnownColorProfile_Srgb: break;                                  // 1 or 2 channels: gray with the sRGB curve
    case KnownColorProfile_LinearSrgb: src.transfer = 8; break;          // 1 or 2 channels: linear gray
    case KnownColorProfile_LinearGray:
    case KnownColorProfile_GraySrgbTRC:
      if (!gray) refuse("a gray colour profile needs 1 or 2 channels");
      if (px->colour == KnownColorProfile_LinearGray) src.transfer = 8;
      break;
    case KnownColorProfile_DisplayP3: src.primaries = 11; break;
    case KnownColorProfile_Rec709: src.transfer = 1; break;
    case KnownColorProfile_Rec2020Linear: src.primaries = 9; src.transfer = 8; break;
    case KnownColorProfile_Rec2020PQ: src.primaries = 9; src.transfer = 16; src.pq = true; break;
    default: refuse("unknown colour profile");
  }
  if (gray && px->colour >= KnownColorProfile_DisplayP3) refuse("an RGB colour profile needs 3 or 4 channels");
  if (md->iccProfile && md->iccProfileSize) refuse("jxlhip_save_pixels signals colour by the KnownColorProfile only: no ICC profile");
  if (opt->lossless && src.exp_bits) refuse("lossless float samples are not supported (save lossy, or as integers)");
}

// The refusals of a JxlHipLossyOptions, on the host
void CheckLossyOptions(const JxlHipLossyOptions* lossy) {
  if (lossy->chroma_from_luma < 0 || lossy->chroma_from_luma > 1)
    throw EncFail(EncoderStatus_EncodeError, "JxlHipLossyOptions: chroma_from_luma must be 0 (maps all zero) or 1 (fitted per tile)");
  for (int32_t r : lossy->reserved)
    if (r) throw EncFail(EncoderStatus_EncodeError, "JxlHipLossyOptions: the reserved words must be zero");
}

}  // namespace

// Part 3 of the C-ABI: SaveImage for every sample type the decoder hands out.  Everything behind the front end is SaveImage's.
extern "C" JXLFILETYPEIO_API EncoderStatus jxlhip_save_pixels_lossy(const JxlHipPixels* pixels, const EncoderOptions* options, const JxlHipLossyOptions* lossy,
                                                                    const EncoderImageMetadata* metadata, IOCallbacks* callbacks, ErrorInfo* err,
                                                                    ProgressProc progress) {
  if (!pixels || !options || !lossy || !callbacks || !metadata) return EncoderStatus_NullParameter;
  try {
    g_last_dist = LastDistances();
    g_last_lossless = JxlHipLosslessInfo();
    EncSource src;
    src.px = pixels;
    CheckPixels(pixels, options, metadata, src);
    CheckLossyOptions(lossy);
    if (!callbacks->Write) throw EncFail(EncoderStatus_NullParameter, "");
    Progress(progress, 0);
    if (options->lossless) EncodeLossless(src, options, metadata, callbacks, progress);
    else EncodeLossy(src, options, *lossy, metadata, callbacks, progress);
    return EncoderStatus_Ok;
  } catch (const EncFail& e) {
    if (e.status == EncoderStatus_EncodeError) SetEncErr(err, e.what());
    return e.status;
  } catch (const std::bad_alloc&) {
    return EncoderStatus_OutOfMemory;
  } catch (const std::exception& e) {
    SetEncErr(err, e.what());
    return EncoderStatus_EncodeError;
  } catch (...) {
    return EncoderStatus_EncodeError;
  }
}

extern "C" JXLFILETYPEIO_API EncoderStatus jxlhip_save_pixels(const JxlHipPixels* pixels, const EncoderOptions* options, const EncoderImageMetadata* metadata,
                                                              IOCallbacks* callbacks, ErrorInfo* err, ProgressProc progress) {
  const JxlHipLossyOptions none = {0, {0, 0, 0}};
  return jxlhip_save_pixels_lossy(pixels, options, &none, metadata, callbacks, err, progress);
}

// =====================================================================================================
// Part 4 of the C-ABI: batch encode of device-resident images.  The flow of EncodeLossy / EncodeLossless reshaped into phases over
// the whole batch ("Batch encode"): the per-image functions above do the work, this only orders it.
// =====================================================================================================
namespace {

constexpr int kEncStreams = 4;        // the front ends of the images are spread over them; the batch kernels use them side by side
constexpr int kEncHostThreads = 16;   // code construction and assembly of independent images (a constant: never the machine's core count)

// fn(i) for i in [0, n) on up to kEncHostThreads threads; the first exception is rethrown on the caller's thread
template <class F>
void ParallelFor(int n, F fn) {
  if (n <= 0) return;
  std::atomic<int> next{0};
  std::exception_ptr failed;
  std::atomic<bool> has_failed{false};
  auto work = [&]() {
    for (int i = next++; i < n; i = next++) {
      try { fn(i); } catch (...) { if (!has_failed.exchange(true)) failed = std::current_exception(); }
    }
  };
  std::vector<std::thread> pool;
  const int nt = std::min(n, kEncHostThreads);
  try {
    for (int t = 1; t < nt; t++) pool.emplace_back(work);
  } catch (...) {}   // fewer threads than wanted: the ones that started, and this one, do the work
  work();
  for (auto& t : pool) t.join();
  if (has_failed) std::rethrow_exception(failed);
}

// Appends `c` to the host image `blob` of a code region that begins at `d_region`; the device view of it.  256-byte alignment of
// every array, as hipMalloc gives the arrays of the single-image path (EncCodeBytes counts it).
EncCodeDev PackEncCode(const EncCode& c, std::vector<uint8_t>& blob, uint8_t* d_region) {
  auto put = [&](const void* p, size_t bytes) {
    const size_t o = (blob.size() + 255) & ~(size_t)255;
    blob.resize(o + bytes);
    if (bytes) memcpy(blob.data() + o, p, bytes);
    return d_region + o;
  };
  EncCodeDev d;
  d.ctx_map = put(c.ctx_map.data(), c.ctx_map.size());
  d.freq = (const uint16_t*)put(c.freq.data(), c.freq.size() * 2);
  d.start = (const uint16_t*)put(c.start.data(), c.start.size() * 2);
  d.rmap = (const uint16_t*)put(c.rmap.data(), c.rmap.size() * 2);
  d.num_clusters = c.num_clusters;
  d.num_ctx = (uint32_t)c.ctx_map.size();
  return d;
}

// pinned host memory that grows to the largest request and is reused
struct PinnedBuffer {
  uint8_t* p = nullptr;
  size_t cap = 0;
  ~PinnedBuffer() { if (p) (void)hipHostFree(p); }
  bool Reserve(size_t bytes) {   // true: it had to grow
    if (bytes <= cap) return false;
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
    const size_t want = bytes + bytes / 4;
    ENC_HIP(hipHostMalloc((void**)&p, want, hipHostMallocDefault));
    cap = want;
    return true;
  }
};
struct DeviceBuffer {
  uint8_t* p = nullptr;
  size_t cap = 0;
  ~DeviceBuffer() { if (p) (void)hipFree(p); }
  bool Reserve(size_t bytes, bool slack) {
    if (bytes <= cap) return false;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    const size_t want = slack ? bytes + bytes / 4 : bytes;
    ENC_HIP(hipMalloc((void**)&p, want));
    cap = want;
    return true;
  }
};

double MsSince(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// one accepted image of a batch
struct BatchJob {
  int index = 0;               // in the caller's arrays
  EncSource src;
  EncoderImageMetadata md;
  EncoderOptions opt;
  bool lossless = false;
  JxlHipLossyOptions lossy = {0, {0, 0, 0}};
  LossyParams qp;
  BitWriter lf_global, hf_global;
  EncCode mcode, acode;
  size_t first_section = 0;    // of the batch's section list
  const FrameOnCanvas* on = nullptr;   // a frame of an animation: the result is the frame alone, no image header, no container
};

}  // namespace

struct JxlHipEncoder {
  int device = 0;
  hipStream_t streams[kEncStreams] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t fork = nullptr, join[kEncStreams] = {nullptr, nullptr, nullptr, nullptr};
  Arena tables;                // the front end's tables, uploaded once
  EncImage table_ptrs;         // an EncImage that holds nothing but their pointers
  DeviceBuffer ws, packed;     // the workspace (enc_batch_layout.h); the compaction's destination
  PinnedBuffer h_hist, h_packed;
  std::vector<std::vector<uint8_t>> files;   // the results of the last batch
  std::vector<std::pair<const char*, float>> stages;
  DeviceBuffer anim;                         // animation encode: the frame table and the extents of the pairs; with a tolerance, one
                                             // frame's tile table and the reference canvas
  std::vector<AnimRect> anim_rects;          // the rectangles of the last animation: per input frame, the bounding box of what it wrote
  struct AnimPart { int32_t k; AnimRect r; };
  std::vector<AnimPart> anim_parts;          // ... per codestream frame: the input frame it belongs to and its rectangle
  std::vector<uint32_t> anim_tiles;          // ... and, with max_rects >= 2 or a tolerance, the tile tables of its pairs (anim_tiles_per_pair words each)
  size_t anim_tiles_per_pair = 0;

  explicit JxlHipEncoder(int dev) {
    if (dev >= 0) ENC_HIP(hipSetDevice(dev));
    ENC_HIP(hipGetDevice(&device));
    try {
      for (auto& s : streams) ENC_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      ENC_HIP(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
      for (auto& e : join) ENC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      memset(&table_ptrs, 0, sizeof(table_ptrs));
      UploadEncTables(tables, table_ptrs);
    } catch (...) {
      Release();
      throw;
    }
  }
  ~JxlHipEncoder() { Release(); }
  JxlHipEncoder(const JxlHipEncoder&) = delete;
  JxlHipEncoder& operator=(const JxlHipEncoder&) = delete;
  void Release() {
    for (auto& s : streams) if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); s = nullptr; }
    if (fork) { (void)hipEventDestroy(fork); fork = nullptr; }
    for (auto& e : join) if (e) { (void)hipEventDestroy(e); e = nullptr; }
  }
  void WaitAll() { for (auto& s : streams) (void)hipStreamSynchronize(s); }
  // streams[to] continues once everything enqueued so far on the streams `from` (a bit mask) is done
  void Join(unsigned from, int to) {
    for (int k = 0; k < kEncStreams; k++) {
      if (!((from >> k) & 1) || k == to) continue;
      ENC_HIP(hipEventRecord(join[k], streams[k]));
      ENC_HIP(hipStreamWaitEvent(streams[to], join[k], 0));
    }
  }
  // every stream continues once everything enqueued so far on streams[from] is done
  void Fork(int from) {
    ENC_HIP(hipEventRecord(fork, streams[from]));
    for (int k = 0; k < kEncStreams; k++) if (k != from) ENC_HIP(hipStreamWaitEvent(streams[k], fork, 0));
  }
  void Run(std::vector<BatchJob>& jobs);
};

// The accepted images of a batch, start to finish.  Throws EncFail for what fails the whole batch (device errors, out of memory).
void JxlHipEncoder::Run(std::vector<BatchJob>& jobs) {
  const int n = (int)jobs.size();
  StageMarks marks;
  std::vector<std::pair<const char*, float>> host_stages;
  auto t0 = std::chrono::steady_clock::now();
  auto host_stage = [&](const char* name) { host_stages.push_back({name, (float)MsSince(t0)}); t0 = std::chrono::steady_clock::now(); };
  hipStream_t s0 = streams[0], s_ans = streams[1], s_ll = streams[2], s_ga = streams[3];
  // ---- 1. geometry, layout, records
  std::vector<EncBatchItem> items((size_t)n);
  for (int i = 0; i < n; i++) {
    const JxlHipPixels& px = *jobs[i].src.px;
    items[i] = EncBatchItem{px.width, px.height, px.num_channels, (int32_t)jobs[i].src.sample_bytes(), jobs[i].lossless ? 1 : 0, jobs[i].lossy.chroma_from_luma};
  }
  std::vector<EncImage> ims((size_t)n);
  EncBatchLayout lay;
  LayEncBatch(items.data(), n, nullptr, ims.data(), &lay);   // measures
  host_stage("host: checks and layout");
  if (ws.Reserve(lay.total_bytes, false)) host_stage("host: workspace allocation");
  LayEncBatch(items.data(), n, ws.p, ims.data(), &lay);      // places
  const size_t hist_bytes = lay.region[kEncSecBits] - lay.region[kEncHist], secbits_bytes = lay.region[kEncCount] - lay.region[kEncSecBits];
  if (h_hist.Reserve(std::max(hist_bytes, secbits_bytes))) host_stage("host: pinned buffer allocation");
  // the tables of the batch kernels: which images each covers, and where each image's share of its grid begins
  const size_t tstride = EncBatchTableStride(n);
  std::vector<uint8_t> up1(lay.records_a - lay.tables, 0);   // host image of the first upload: tables | records | Modular codes
  enum { kTabReverseMod = 0, kTabReverseHf = 1, kTabSections = 2, kTabLl = 3, kTabGlobalAlpha = 4, kTabCompact = 5 };
  EncBatchTable tab[kEncBatchTables];
  uint32_t units[kEncBatchTables] = {0, 0, 0, 0, 0, 0};
  const int per_wg = EncSectionsPerWg();
  for (int t = 0; t < kEncBatchTables; t++) {
    uint32_t* first = (uint32_t*)(up1.data() + (size_t)(3 * t) * tstride);
    int32_t* image_of = (int32_t*)(up1.data() + (size_t)(3 * t + 1) * tstride);
    uint32_t* wg0 = (uint32_t*)(up1.data() + (size_t)(3 * t + 2) * tstride);
    int entries = 0;
    auto add = [&](int i, uint32_t from, uint32_t to) {   // workgroups [from, to) of image i
      if (to <= from) return;
      first[entries] = units[t]; image_of[entries] = i; wg0[entries] = from;
      entries++;
      units[t] += to - from;
    };
    // the streams of a lossy frame are numbered LF groups first (encode_kernels.hip: LossyStream): these workgroups hold its LF streams
    auto lf_wgs = [&](const EncImage& im) { return (uint32_t)((2 * im.nlf + per_wg - 1) / per_wg); };
    auto reverse_wgs = [&](const EncImage& im) { return (uint32_t)((2 * (im.nlf + im.ng) + per_wg - 1) / per_wg); };
    if (t == kTabReverseMod) {
      // the LF coefficients of an LF group are the longest recurrence of a frame: those of every image start first, side by side
      for (int i = 0; i < n; i++) if (!ims[i].lossless) add(i, 0, std::min(lf_wgs(ims[i]), reverse_wgs(ims[i])));
      for (int i = 0; i < n; i++) if (!ims[i].lossless) add(i, std::min(lf_wgs(ims[i]), reverse_wgs(ims[i])), reverse_wgs(ims[i]));
    } else {
      for (int i = 0; i < n; i++) {
        const EncImage& im = ims[i];
        switch (t) {
          case kTabReverseHf: if (!im.lossless) add(i, 0, reverse_wgs(im)); break;
          case kTabSections: if (!im.lossless) add(i, 0, (uint32_t)((im.nlf + im.ng + per_wg - 1) / per_wg)); break;
          case kTabLl: if (im.lossless) add(i, 0, (uint32_t)((im.ng + per_wg - 1) / per_wg)); break;
          case kTabGlobalAlpha: if (!im.lossless && im.has_alpha && im.ng == 1) add(i, 0, 1); break;
          default: add(i, 0, (uint32_t)EncNumSections(im)); break;
        }
      }
    }
    tab[t].first = (const uint32_t*)(ws.p + lay.tables + (size_t)(3 * t) * tstride);
    tab[t].image_of = (const int32_t*)(ws.p + lay.tables + (size_t)(3 * t + 1) * tstride);
    tab[t].wg0 = (const uint32_t*)(ws.p + lay.tables + (size_t)(3 * t + 2) * tstride);
    tab[t].entries = entries; tab[t].pad = 0;
  }
  {
    size_t sec = 0;
    for (int i = 0; i < n; i++) { jobs[i].first_section = sec; sec += (size_t)EncNumSections(ims[i]); }
  }
  host_stage("host: records and tables");
  // ---- 2. per image, spread over the streams: pixels into tight rows, front end, tokens and histograms
  ENC_HIP(hipMemsetAsync(ws.p, 0, lay.head_bytes, s0));   // every counter and histogram of the batch
  Fork(0);
  const size_t k_front = marks.Begin("pixels, front end, tokens + histograms (per image, on four streams)", s0);
  for (int i = 0; i < n; i++) {
    BatchJob& job = jobs[i];
    EncImage& im = ims[i];
    hipStream_t s = streams[i % kEncStreams];
    const JxlHipPixels& px = *job.src.px;
    const size_t row = (size_t)px.width * px.num_channels * job.src.sample_bytes();
    uint8_t* d_src = ws.p + lay.slots[i].src;
    // tight, 256-byte aligned rows whatever the caller's pointer and stride are: what the loaders of encode_kernels.hip rely on
    ENC_HIP(hipMemcpy2DAsync(d_src, row, px.data, px.stride_bytes, row, px.height, hipMemcpyDeviceToDevice, s));
    SetPixelSource(job.src, d_src, ws.p + lay.slots[i].surface, im, s);
    if (job.lossless) {
      im.ll_rct = im.gray ? 0 : 1;
      im.ll_tok_extra = 0;
      LaunchEncLossless(im, 0, s);
    } else {
      job.qp = SetLossyParams(&job.opt, im);
      CopyEncTables(table_ptrs, im);
      LaunchEncFrontEnd(im, s);
      LaunchEncTokens(im, s);
    }
  }
  Join(~0u, 0);
  marks.End(k_front, s0);
  { const size_t k = marks.Begin("histogram download (one copy)", s0); ENC_HIP(hipMemcpyAsync(h_hist.p, ws.p + lay.region[kEncHist], hist_bytes, hipMemcpyDeviceToHost, s0)); marks.End(k, s0); }
  ENC_HIP(hipStreamSynchronize(s0));   // the one synchronisation before the codes
  host_stage("host: enqueue and wait for the histograms");
  auto host_hist = [&](const uint32_t* dev) { return (const uint32_t*)(h_hist.p + ((const uint8_t*)dev - (ws.p + lay.region[kEncHist]))); };
  // ---- 3a. the Modular codes of every image; up they go with the records, and the recurrences that need nothing else start
  ParallelFor(n, [&](int i) {
    BatchJob& job = jobs[i];
    if (job.lossless) WriteLosslessFixedGlobal(ims[i], host_hist(ims[i].hist_mod), job.lf_global, job.mcode);
    else WriteLossyLfGlobal(ims[i], job.qp, host_hist(ims[i].hist_mod), job.lf_global, job.mcode);
  });
  host_stage("host: Modular code construction");
  size_t lds_m = 0, lds_ll = 0;
  {
    std::vector<uint8_t> blob;
    for (int i = 0; i < n; i++) {
      ims[i].mcode = PackEncCode(jobs[i].mcode, blob, ws.p + lay.mcodes);
      size_t& lds = jobs[i].lossless ? lds_ll : lds_m;
      lds = std::max(lds, EncReverseLds(ims[i].mcode.num_clusters, ims[i].mcode.num_ctx, 0));
    }
    if (blob.size() > lay.records_a - lay.mcodes) throw EncFail(EncoderStatus_EncodeError, "the Modular codes outgrew their room");
    memcpy(up1.data() + (lay.records_m - lay.tables), ims.data(), (size_t)n * sizeof(EncImage));
    memcpy(up1.data() + (lay.mcodes - lay.tables), blob.data(), blob.size());
    ENC_HIP(hipMemcpyAsync(ws.p + lay.tables, up1.data(), (lay.mcodes - lay.tables) + blob.size(), hipMemcpyHostToDevice, s_ans));
  }
  const EncImage* d_ims_m = (const EncImage*)(ws.p + lay.records_m);
  const EncImage* d_ims_a = (const EncImage*)(ws.p + lay.records_a);
  Fork(1);
  { const size_t k = marks.Begin("reverse pass, Modular streams of every image (one launch)", s_ans); LaunchEncReverseBatch(d_ims_m, tab[kTabReverseMod], units[kTabReverseMod], 0, lds_m, s_ans); marks.End(k, s_ans); }
  { const size_t k = marks.Begin("lossless sections of every image (one launch)", s_ll); LaunchEncLlSectionsBatch(d_ims_m, tab[kTabLl], units[kTabLl], lds_ll, s_ll); marks.End(k, s_ll); }
  { const size_t k = marks.Begin("global alpha sections (one launch)", s_ga); LaunchEncGlobalAlphaBatch(d_ims_m, tab[kTabGlobalAlpha], s_ga); marks.End(k, s_ga); }
  host_stage("host: Modular code upload and launches");
  // ---- 3b. the HF codes, built while the Modular streams' recurrences run
  std::vector<int> lossy;
  for (int i = 0; i < n; i++) if (!jobs[i].lossless) lossy.push_back(i);
  ParallelFor((int)lossy.size(), [&](int k) {
    const int i = lossy[k];
    WriteLossyHfGlobal(ims[i], host_hist(ims[i].hist_ac), jobs[i].hf_global, jobs[i].acode);
  });
  host_stage("host: HF code construction");
  size_t lds_a = 0;
  {
    std::vector<uint8_t> up2(lay.acodes - lay.records_a, 0);   // records | HF codes
    std::vector<uint8_t> blob;
    for (int i : lossy) {
      ims[i].acode = PackEncCode(jobs[i].acode, blob, ws.p + lay.acodes);
      lds_a = std::max(lds_a, EncReverseLds(ims[i].acode.num_clusters, ims[i].acode.num_ctx, 1));
    }
    if (blob.size() > lay.dst_off - lay.acodes) throw EncFail(EncoderStatus_EncodeError, "the HF codes outgrew their room");
    memcpy(up2.data(), ims.data(), (size_t)n * sizeof(EncImage));
    up2.insert(up2.end(), blob.begin(), blob.end());
    ENC_HIP(hipMemcpyAsync(ws.p + lay.records_a, up2.data(), up2.size(), hipMemcpyHostToDevice, s0));
    ENC_HIP(hipStreamSynchronize(s0));   // up2 leaves scope; the copy from pageable memory has been staged by then anyway
  }
  // ---- 4. reverse passes of the HF streams, bit layout of every section, compaction, download
  { const size_t k = marks.Begin("reverse pass, HF streams of every image (one launch)", s0); LaunchEncReverseBatch(d_ims_a, tab[kTabReverseHf], units[kTabReverseHf], 1, lds_a, s0); marks.End(k, s0); }
  Join(1u << 1, 0);   // the section layout needs the states of both kinds of stream
  { const size_t k = marks.Begin("section bit layout of every image (one launch)", s0); LaunchEncSectionsBatch(d_ims_a, tab[kTabSections], units[kTabSections], s0); marks.End(k, s0); }
  Join((1u << 2) | (1u << 3), 0);
  ENC_HIP(hipMemcpyAsync(h_hist.p, ws.p + lay.region[kEncSecBits], secbits_bytes, hipMemcpyDeviceToHost, s0));
  ENC_HIP(hipStreamSynchronize(s0));
  host_stage("host: HF code upload, launches and wait for the sections");
  auto host_bits = [&](const uint64_t* dev) { return (const uint64_t*)(h_hist.p + ((const uint8_t*)dev - (ws.p + lay.region[kEncSecBits]))); };
  std::vector<uint64_t> off(lay.total_sections + 1, 0);
  for (int i = 0; i < n; i++) {
    const uint64_t* bits = host_bits(ims[i].sec_bits);
    const int nsec = EncNumSections(ims[i]);
    for (int k = 0; k < nsec; k++) off[jobs[i].first_section + k + 1] = off[jobs[i].first_section + k] + ((bits[k] + 7) >> 3);
  }
  const size_t packed_bytes = std::max<uint64_t>(off[lay.total_sections], 1);
  {
    const bool grew_d = packed.Reserve(packed_bytes, true), grew_h = h_packed.Reserve(packed_bytes);
    if (grew_d || grew_h) host_stage("host: output buffer allocation");
  }
  ENC_HIP(hipMemcpyAsync(ws.p + lay.dst_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, s0));
  { const size_t k = marks.Begin("compaction of every section (one launch)", s0); LaunchEncCompactBatch(d_ims_a, tab[kTabCompact], units[kTabCompact], (const uint64_t*)(ws.p + lay.dst_off), packed.p, s0); marks.End(k, s0); }
  { const size_t k = marks.Begin("section download (one copy)", s0); ENC_HIP(hipMemcpyAsync(h_packed.p, packed.p, packed_bytes, hipMemcpyDeviceToHost, s0)); marks.End(k, s0); }
  ENC_HIP(hipStreamSynchronize(s0));
  ENC_HIP(hipGetLastError());
  host_stage("host: compaction and download");
  // ---- 5. codestream and container of every image
  ParallelFor(n, [&](int i) {
    BatchJob& job = jobs[i];
    const uint64_t* o = off.data() + job.first_section;
    const uint64_t* bits = host_bits(ims[i].sec_bits);
    if (job.on) {
      EncFrameInfo fi = job.qp.fi;
      fi.at = job.on->at;
      files[(size_t)job.index] = job.lossless ? AssembleLossless(ims[i], job.src, &job.md, job.lf_global, h_packed.p, o, bits, job.on)
                                              : AssembleLossy(ims[i], job.on->canvas, fi, job.lf_global, job.hf_global, h_packed.p, o, bits, true);
      return;
    }
    const std::vector<uint8_t> cs = job.lossless ? AssembleLossless(ims[i], job.src, &job.md, job.lf_global, h_packed.p, o, bits)
                                                 : AssembleLossy(ims[i], DescribeImage(ims[i], job.src, &job.md, true), job.qp.fi, job.lf_global, job.hf_global, h_packed.p, o, bits);
    files[(size_t)job.index] = WriteContainer(cs, job.md.exif, job.md.exifSize, job.md.xmp, job.md.xmpSize);
  });
  host_stage("host: assembly");
  marks.Publish(&stages);
  stages.insert(stages.end(), host_stages.begin(), host_stages.end());
}

extern "C" JXLFILETYPEIO_API JxlHipEncoder* jxlhip_encoder_create(int32_t device, ErrorInfo* err) {
  try {
    return new JxlHipEncoder(device);
  } catch (const std::exception& e) {
    SetEncErr(err, e.what());
    return nullptr;
  } catch (...) {
    return nullptr;
  }
}

extern "C" JXLFILETYPEIO_API void jxlhip_encoder_destroy(JxlHipEncoder* enc) { delete enc; }

namespace {
// What a batch refuses of an image, on the host (jxlhip_encode_batch per image, jxlhip_encode_animation per frame)
void CheckBatchImage(const JxlHipPixels* px, const EncoderOptions* opt, const EncoderImageMetadata* md, EncSource& src) {
  CheckPixels(px, opt, md, src);
  if (opt->effort >= 8)
    throw EncFail(EncoderStatus_EncodeError, "efforts 8 and 9 (the closed loop and the lossless search) are not available in a batch: use jxlhip_save_pixels");
}
}  // namespace

extern "C" JXLFILETYPEIO_API EncoderStatus jxlhip_encode_batch(JxlHipEncoder* enc, int32_t n, const JxlHipPixels* images, const EncoderOptions* options,
                                                               const EncoderImageMetadata* const* metadata, EncoderStatus* statuses, ErrorInfo* err) {
  return jxlhip_encode_batch_lossy(enc, n, images, options, nullptr, metadata, statuses, err);
}

extern "C" JXLFILETYPEIO_API EncoderStatus jxlhip_encode_batch_lossy(JxlHipEncoder* enc, int32_t n, const JxlHipPixels* images, const EncoderOptions* options,
                                                                     const JxlHipLossyOptions* lossy, const EncoderImageMetadata* const* metadata,
                                                                     EncoderStatus* statuses, ErrorInfo* err) {
  if (!enc || n < 0 || (n > 0 && (!images || !options || !statuses))) return EncoderStatus_NullParameter;
  enc->files.assign((size_t)n, std::vector<uint8_t>());
  enc->stages.clear();
  EncoderStatus first = EncoderStatus_Ok;
  auto report = [&](int i, EncoderStatus st, const char* what) {
    if (first != EncoderStatus_Ok) return;
    first = st;
    if (st != EncoderStatus_EncodeError) return;
    char msg[256];
    snprintf(msg, sizeof(msg), "image %d: %s", i, what);
    SetEncErr(err, msg);
  };
  // the refusals, per image, on the host, before any device work
  std::vector<BatchJob> jobs;
  jobs.reserve((size_t)n);
  for (int i = 0; i < n; i++) {
    statuses[i] = EncoderStatus_Ok;
    BatchJob job;
    job.index = i;
    job.src.px = &images[i];
    job.opt = options[i];
    memset(&job.md, 0, sizeof(job.md));
    if (metadata && metadata[i]) job.md = *metadata[i];
    try {
      CheckBatchImage(&images[i], &options[i], &job.md, job.src);
      if (lossy) { CheckLossyOptions(&lossy[i]); job.lossy = lossy[i]; }
      job.lossless = options[i].lossless;
      jobs.push_back(std::move(job));
    } catch (const EncFail& e) {
      statuses[i] = e.status;
      report(i, e.status, e.what());
    }
  }
  if (jobs.empty()) return first;
  EncoderStatus failed = EncoderStatus_Ok;
  std::string why;
  int caller_device = enc->device;   // the calling thread's current device is restored before the call returns
  (void)hipGetDevice(&caller_device);
  try {
    if (caller_device != enc->device) ENC_HIP(hipSetDevice(enc->device));
    enc->Run(jobs);
  } catch (const EncFail& e) {
    failed = e.status; why = e.what();
  } catch (const std::bad_alloc&) {
    failed = EncoderStatus_OutOfMemory;
  } catch (const std::exception& e) {
    failed = EncoderStatus_EncodeError; why = e.what();
  } catch (...) {
    failed = EncoderStatus_EncodeError;   // never throw across the ABI
  }
  if (failed != EncoderStatus_Ok) {
    // what fails on the device fails the batch: every accepted image reports it, and the encoder is left idle and usable
    enc->WaitAll();
    (void)hipGetLastError();
    for (auto& job : jobs) { statuses[job.index] = failed; enc->files[(size_t)job.index].clear(); }
    if (first == EncoderStatus_Ok) { first = failed; if (failed == EncoderStatus_EncodeError) SetEncErr(err, ("the batch: " + why).c_str()); }
  }
  if (caller_device != enc->device) (void)hipSetDevice(caller_device);
  return first;
}

// =====================================================================================================
// Part 6 of the C-ABI: animation encode.  The extents kernel - with max_rects >= 2 the tile kernel - says what
// changed, enc_animation.cc turns that into rectangles, one per frame or several, and the rectangles go through Run like the images
// of a batch - a crop is a pointer offset and a narrower row in Run's copy into tight rows.  Run hands back every frame alone (header,
// TOC, sections); they follow the image header in one codestream.  With a tolerance for "unchanged" the measuring is a loop over the
// frames against a reference canvas instead (EncodeAnimation, step 2); everything behind the rectangles is the same.
// =====================================================================================================
namespace {

constexpr int kAnimMaxChunkFrames = 64;                      // frames of one Run unless chunk_frames says otherwise
constexpr size_t kAnimWorkspaceBudget = (size_t)32 << 30;    // ... and at most this much workspace (32 4K RGBA frames), unless one frame needs more

// Everything behind the host's checks.  src0: what CheckPixels made of frame 0 (the same for every frame).
void EncodeAnimation(JxlHipEncoder* enc, int32_t n, const JxlHipPixels* frames, const uint32_t* durations, const EncoderOptions& opt,
                     const JxlHipAnimationOptions& ao, const JxlHipAnimationRectOptions& ro, const JxlHipAnimationChangeOptions& co,
                     const EncoderImageMetadata& md, const EncSource& src0) {
  const JxlHipPixels& f0 = frames[0];
  const int32_t w = (int32_t)f0.width, h = (int32_t)f0.height;
  const uint32_t pixel_bytes = (uint32_t)(f0.num_channels * src0.sample_bytes());
  const bool lossless = opt.lossless;
  const bool by_tiles = ro.max_rects >= 2;
  hipStream_t s0 = enc->streams[0];
  StageMarks marks;
  // ---- 1. what changed between consecutive frames: one launch and one download - 16 bytes per pair (max_rects = 1: its box), or
  // 4 bytes per pair and 64 x 64 tile.  With a tolerance (further down) frame k is measured against the reference canvas instead, a
  // launch per frame, and its rectangles are found before frame k + 1 is measured
  std::vector<AnimExtent> ext((size_t)std::max(n - 1, 0));
  const size_t tiles_per_pair = (size_t)AnimTilesAcross(w) * AnimTilesAcross(h);
  const bool with_tolerance = co.tolerance > 0.f;
  if (n > 1 && !with_tolerance) {
    const size_t table_bytes = ((size_t)n * sizeof(AnimFrameSrc) + 255) & ~(size_t)255;
    const size_t out_bytes = by_tiles ? ext.size() * tiles_per_pair * sizeof(uint32_t) : ext.size() * sizeof(AnimExtent);
    enc->anim.Reserve(table_bytes + out_bytes, true);
    std::vector<AnimFrameSrc> table((size_t)n);
    for (int k = 0; k < n; k++) table[(size_t)k] = AnimFrameSrc{(const uint8_t*)frames[k].data, (int64_t)frames[k].stride_bytes};
    ENC_HIP(hipMemcpyAsync(enc->anim.p, table.data(), table.size() * sizeof(AnimFrameSrc), hipMemcpyHostToDevice, s0));
    if (by_tiles) {
      uint32_t* d_tiles = (uint32_t*)(enc->anim.p + table_bytes);
      enc->anim_tiles.resize(ext.size() * tiles_per_pair);
      enc->anim_tiles_per_pair = tiles_per_pair;
      const size_t k_tiles = marks.Begin("change tiles of every pair of frames (one launch)", s0);
      LaunchAnimTiles((const AnimFrameSrc*)enc->anim.p, n - 1, w, h, pixel_bytes, d_tiles, s0);
      marks.End(k_tiles, s0);
      ENC_HIP(hipMemcpyAsync(enc->anim_tiles.data(), d_tiles, out_bytes, hipMemcpyDeviceToHost, s0));
    } else {
      AnimExtent* d_ext = (AnimExtent*)(enc->anim.p + table_bytes);
      ENC_HIP(hipMemsetAsync(d_ext, 0xFF, out_bytes, s0));
      const size_t k_ext = marks.Begin("change extents of every pair of frames (one launch)", s0);
      LaunchAnimExtents((const AnimFrameSrc*)enc->anim.p, n - 1, h, (uint64_t)f0.width * pixel_bytes, pixel_bytes, d_ext, s0);
      marks.End(k_ext, s0);
      ENC_HIP(hipMemcpyAsync(ext.data(), d_ext, out_bytes, hipMemcpyDeviceToHost, s0));
    }
    ENC_HIP(hipStreamSynchronize(s0));   // (also: `table` was staged)
    ENC_HIP(hipGetLastError());
    if (by_tiles)
      for (size_t p = 0; p < ext.size(); p++) ext[p] = AnimTilesExtent(enc->anim_tiles.data() + p * tiles_per_pair, w, h);
  }
  // ---- 2. the rectangles and what the headers say: a frame with m rectangles is m codestream frames, of which the last carries the
  // duration (the others have none: the decoder composes them into the next displayed image)
  EncImageInfo canvas;
  canvas.xsize = f0.width; canvas.ysize = f0.height;
  canvas.gray = f0.num_channels < 3; canvas.alpha = !(f0.num_channels & 1); canvas.xyb = !lossless;
  src0.Describe(canvas);
  canvas.have_animation = true;
  canvas.tps_numerator = ao.tps_numerator; canvas.tps_denominator = ao.tps_denominator; canvas.num_loops = ao.num_loops;
  enc->anim_rects.resize((size_t)n);
  std::vector<JxlHipEncoder::AnimPart>& parts = enc->anim_parts;
  std::vector<size_t> last_part((size_t)n);   // of frame k: the codestream frame that carries its duration
  // the rectangles of frame k, from ext[k - 1] and the tile table of its pair
  auto place = [&](int k) {
    enc->anim_rects[(size_t)k] = AnimFrameRect(k, ao.key_interval, k ? ext[(size_t)k - 1] : AnimExtent{-1, -1, -1, -1}, w, h, lossless);
    if (by_tiles && !AnimIsKeyFrame(k, ao.key_interval)) {
      for (const AnimRect& r : AnimFrameRects(enc->anim_tiles.data() + (size_t)(k - 1) * tiles_per_pair, w, h, lossless, ro.max_rects, ro.merge_pixels))
        parts.push_back(JxlHipEncoder::AnimPart{k, r});
    } else {
      parts.push_back(JxlHipEncoder::AnimPart{k, enc->anim_rects[(size_t)k]});
    }
    last_part[(size_t)k] = parts.size() - 1;
  };
  if (!with_tolerance) {
    for (int k = 0; k < n; k++) place(k);
  } else {
    // With a tolerance: the reference canvas R holds the source of what a decoder shows - frame 0, then frame k's pixels inside every
    // rectangle frame k is written as (lossy: the grown ones; the 1 x 1 of an unchanged frame too).  Frame k is measured against R, per
    // tile whatever max_rects is (max_rects = 1 reduces the table to its box; a key frame is measured too, then R is the frame), the
    // host turns the table into rectangles, and R takes them before frame k + 1 is measured: a round trip per frame.
    place(0);
    if (n > 1) {
      const AnimSample kind = src0.exp_bits == 8 ? kAnimF32 : (src0.exp_bits ? kAnimF16 : (src0.sample_bytes() == 2 ? kAnimU16 : kAnimU8));
      const size_t table_bytes = (tiles_per_pair * sizeof(uint32_t) + 255) & ~(size_t)255;
      const uint64_t row_bytes = (uint64_t)f0.width * pixel_bytes;
      enc->anim.Reserve(table_bytes + (size_t)(row_bytes * (uint64_t)h), true);
      uint32_t* d_tiles = (uint32_t*)enc->anim.p;
      uint8_t* ref = enc->anim.p + table_bytes;
      enc->anim_tiles.resize(ext.size() * tiles_per_pair);
      enc->anim_tiles_per_pair = tiles_per_pair;
      auto src_of = [&](int k) { return AnimFrameSrc{(const uint8_t*)frames[k].data, (int64_t)frames[k].stride_bytes}; };
      std::vector<AnimRect> rects;
      const size_t k_loop = marks.Begin("change tiles against the reference canvas (a launch per frame)", s0);
      LaunchAnimApplyRects(src_of(0), ref, w, pixel_bytes, &enc->anim_rects[0], 1, s0);
      for (int k = 1; k < n; k++) {
        uint32_t* tiles = enc->anim_tiles.data() + (size_t)(k - 1) * tiles_per_pair;
        LaunchAnimTilesTol(src_of(k), ref, w, h, pixel_bytes, kind, co.tolerance, d_tiles, s0);
        ENC_HIP(hipMemcpyAsync(tiles, d_tiles, tiles_per_pair * sizeof(uint32_t), hipMemcpyDeviceToHost, s0));
        ENC_HIP(hipStreamSynchronize(s0));
        ENC_HIP(hipGetLastError());
        ext[(size_t)k - 1] = AnimTilesExtent(tiles, w, h);
        const size_t first = parts.size();
        place(k);
        rects.clear();
        for (size_t c = first; c < parts.size(); c++) rects.push_back(parts[c].r);
        LaunchAnimApplyRects(src_of(k), ref, w, pixel_bytes, rects.data(), (int32_t)rects.size(), s0);
      }
      marks.End(k_loop, s0);
      ENC_HIP(hipStreamSynchronize(s0));
      ENC_HIP(hipGetLastError());
    }
  }
  const int total = (int)parts.size();
  std::vector<FrameOnCanvas> on((size_t)total);
  std::vector<JxlHipPixels> crops((size_t)total);
  for (int c = 0; c < total; c++) {
    const int k = parts[(size_t)c].k;
    const AnimRect& r = parts[(size_t)c].r;
    on[(size_t)c].canvas = canvas;
    on[(size_t)c].at = AnimPlacement(c, total, r, w, h, (size_t)c == last_part[(size_t)k] ? durations[k] : 0);
    JxlHipPixels& px = crops[(size_t)c];
    px = frames[k];
    px.data = (const uint8_t*)frames[k].data + (size_t)r.y * frames[k].stride_bytes + (size_t)r.x * pixel_bytes;
    px.width = (uint32_t)r.w; px.height = (uint32_t)r.h;
  }
  // ---- 3. the frames, a chunk at a time
  enc->files.assign((size_t)total, std::vector<uint8_t>());
  std::vector<std::pair<const char*, float>> first_stages;
  marks.Publish(&first_stages);
  for (int first = 0; first < total;) {
    int cnt = 0;
    if (ao.chunk_frames >= 1) {
      cnt = std::min(ao.chunk_frames, total - first);
    } else {
      std::vector<EncBatchItem> items;
      std::vector<EncImage> ims;
      EncBatchLayout lay;
      while (first + cnt < total && cnt < kAnimMaxChunkFrames) {
        const JxlHipPixels& c = crops[(size_t)(first + cnt)];
        items.push_back(EncBatchItem{c.width, c.height, c.num_channels, (int32_t)src0.sample_bytes(), lossless ? 1 : 0, 0});
        ims.resize(items.size());
        LayEncBatch(items.data(), (int)items.size(), nullptr, ims.data(), &lay);
        if (cnt > 0 && lay.total_bytes > kAnimWorkspaceBudget) break;
        cnt++;
      }
    }
    std::vector<BatchJob> jobs((size_t)cnt);
    for (int j = 0; j < cnt; j++) {
      BatchJob& job = jobs[(size_t)j];
      job.index = first + j;
      job.src = src0;
      job.src.px = &crops[(size_t)(first + j)];
      job.opt = opt;
      job.md = md;
      job.lossless = lossless;
      job.on = &on[(size_t)(first + j)];
    }
    enc->Run(jobs);
    first += cnt;
  }
  // ---- 4. one codestream: the image header, then every frame; one container
  BitWriter hdr;
  WriteCodestreamHeaders(canvas, hdr);
  const std::vector<uint8_t> head = hdr.Finish();
  size_t cs_size = head.size();
  for (auto& f : enc->files) cs_size += f.size();
  std::vector<uint8_t> file = WriteContainerPrefix(cs_size, md.exif, md.exifSize, md.xmp, md.xmpSize);
  file.reserve(file.size() + cs_size);   // the frames are copied once
  file.insert(file.end(), head.begin(), head.end());
  for (auto& f : enc->files) { file.insert(file.end(), f.begin(), f.end()); std::vector<uint8_t>().swap(f); }
  enc->files.assign(1, std::vector<uint8_t>());
  enc->files[0] = std::move(file);
  enc->stages.insert(enc->stages.begin(), first_stages.begin(), first_stages.end());   // the extents pass, then the last chunk's stages
}

}  // namespace

extern "C" JXLFILETYPEIO_API EncoderStatus jxlhip_encode_animation_changes(JxlHipEncoder* enc, int32_t n, const JxlHipPixels* frames, const uint32_t* durations,
                                                                           const EncoderOptions* options, const JxlHipAnimationOptions* animation,
                                                                           const JxlHipAnimationRectOptions* rects, const JxlHipAnimationChangeOptions* changes,
                                                                           const EncoderImageMetadata* metadata, ErrorInfo* err) {
  if (!enc || !options || !animation || !rects || !changes) return EncoderStatus_NullParameter;
  enc->files.clear();
  enc->stages.clear();
  enc->anim_rects.clear();
  enc->anim_parts.clear();
  enc->anim_tiles.clear();
  enc->anim_tiles_per_pair = 0;
  EncoderImageMetadata md;
  memset(&md, 0, sizeof(md));
  if (metadata) md = *metadata;
  EncSource src0;
  // the refusals, on the host, before any device work
  try {
    auto refuse = [](const std::string& why) { throw EncFail(EncoderStatus_EncodeError, why); };
    if (n < 1) refuse("an animation needs at least one frame");
    if (!frames || !durations) throw EncFail(EncoderStatus_NullParameter, "");
    if (animation->tps_denominator < 1 || animation->tps_denominator > 1024) refuse("the denominator of the ticks per second must be 1..1024");
    if (animation->tps_numerator < 1 || animation->tps_numerator > (1u << 30)) refuse("the numerator of the ticks per second must be 1..2^30");
    if (const char* why = AnimRectOptionsRefusal(rects->max_rects, rects->merge_pixels)) refuse(why);
    if (const char* why = AnimToleranceRefusal(changes->tolerance)) refuse(why);
    for (int k = 0; k < n; k++) {
      const std::string who = "frame " + std::to_string(k) + ": ";
      EncSource src;
      src.px = &frames[k];
      try {
        CheckBatchImage(&frames[k], options, &md, src);
      } catch (const EncFail& e) {
        throw EncFail(e.status, who + e.what());
      }
      if (k == 0) src0 = src;
      const JxlHipPixels &a = frames[0], &b = frames[k];
      if (a.width != b.width || a.height != b.height) refuse(who + "its size differs from frame 0's");
      if (a.num_channels != b.num_channels) refuse(who + "its number of channels differs from frame 0's");
      if (a.sample_type != b.sample_type) refuse(who + "its sample type differs from frame 0's");
      if (a.bits_per_sample != b.bits_per_sample) refuse(who + "its bits per sample differ from frame 0's");
      if (a.colour != b.colour) refuse(who + "its colour profile differs from frame 0's");
      if (durations[k] == 0) refuse(who + "a duration of 0 ticks (every frame is a displayed image and needs one)");
    }
  } catch (const EncFail& e) {
    if (e.status == EncoderStatus_EncodeError) SetEncErr(err, e.what());
    return e.status;
  } catch (...) {
    return EncoderStatus_EncodeError;
  }
  EncoderStatus failed = EncoderStatus_Ok;
  std::string why;
  int caller_device = enc->device;
  (void)hipGetDevice(&caller_device);
  try {
    if (caller_device != enc->device) ENC_HIP(hipSetDevice(enc->device));
    EncodeAnimation(enc, n, frames, durations, *options, *animation, *rects, *changes, md, src0);
  } catch (const EncFail& e) {
    failed = e.status; why = e.what();
  } catch (const std::bad_alloc&) {
    failed = EncoderStatus_OutOfMemory;
  } catch (const std::exception& e) {
    failed = EncoderStatus_EncodeError; why = e.what();
  } catch (...) {
    failed = EncoderStatus_EncodeError;   // never throw across the ABI
  }
  if (failed != EncoderStatus_Ok) {
    enc->WaitAll();
    (void)hipGetLastError();
    enc->files.clear();
    if (failed == EncoderStatus_EncodeError) SetEncErr(err, ("the animation: " + why).c_str());
  }
  if (caller_device != enc->device) (void)hipSetDevice(caller_device);
  return failed;
}

extern "C" JXLFILETYPEIO_API EncoderStatus jxlhip_encode_animation_rects(JxlHipEncoder* enc, int32_t n, const JxlHipPixels* frames, const uint32_t* durations,
                                                                         const EncoderOptions* options, const JxlHipAnimationOptions* animation,
                                                                         const JxlHipAnimationRectOptions* rects, const EncoderImageMetadata* metadata,
                                                                         ErrorInfo* err) {
  const JxlHipAnimationChangeOptions bits = {0.f};
  return jxlhip_encode_animation_changes(enc, n, frames, durations, options, animation, rects, &bits, metadata, err);
}

extern "C" JXLFILETYPEIO_API EncoderStatus jxlhip_encode_animation(JxlHipEncoder* enc, int32_t n, const JxlHipPixels* frames, const uint32_t* durations,
                                                                   const EncoderOptions* options, const JxlHipAnimationOptions* animation,
                                                                   const EncoderImageMetadata* metadata, ErrorInfo* err) {
  const JxlHipAnimationRectOptions one = {1, 0};
  return jxlhip_encode_animation_rects(enc, n, frames, durations, options, animation, &one, metadata, err);
}

extern "C" JXLFILETYPEIO_API int32_t jxlhip_encoder_animation_frame_rects(JxlHipEncoder* enc, int32_t* kxywh, int32_t capacity) {
  if (!enc) return 0;
  const int32_t n = (int32_t)enc->anim_parts.size();
  for (int32_t c = 0; kxywh && c < n && c < capacity; c++) {
    const JxlHipEncoder::AnimPart& p = enc->anim_parts[(size_t)c];
    kxywh[5 * c] = p.k; kxywh[5 * c + 1] = p.r.x; kxywh[5 * c + 2] = p.r.y; kxywh[5 * c + 3] = p.r.w; kxywh[5 * c + 4] = p.r.h;
  }
  return n;
}

extern "C" JXLFILETYPEIO_API int32_t jxlhip_encoder_animation_tiles(JxlHipEncoder* enc, int32_t pair, uint32_t* dst, int32_t capacity) {
  if (!enc || pair < 0 || enc->anim_tiles_per_pair == 0 || (size_t)pair >= enc->anim_tiles.size() / enc->anim_tiles_per_pair) return 0;
  const size_t n = enc->anim_tiles_per_pair;
  for (size_t t = 0; dst && t < n && t < (size_t)std::max(capacity, 0); t++) dst[t] = enc->anim_tiles[(size_t)pair * n + t];
  return (int32_t)n;
}

extern "C" JXLFILETYPEIO_API int32_t jxlhip_encoder_animation_rects(JxlHipEncoder* enc, int32_t* xywh, int32_t capacity) {
  if (!enc) return 0;
  const int32_t n = (int32_t)enc->anim_rects.size();
  for (int32_t k = 0; xywh && k < n && k < capacity; k++) {
    const AnimRect& r = enc->anim_rects[(size_t)k];
    xywh[4 * k] = r.x; xywh[4 * k + 1] = r.y; xywh[4 * k + 2] = r.w; xywh[4 * k + 3] = r.h;
  }
  return n;
}

extern "C" JXLFILETYPEIO_API int32_t jxlhip_encoder_result(JxlHipEncoder* enc, int32_t i, const uint8_t** data, size_t* size) {
  if (!enc || i < 0 || (size_t)i >= enc->files.size() || enc->files[(size_t)i].empty()) return 0;
  if (data) *data = enc->files[(size_t)i].data();
  if (size) *size = enc->files[(size_t)i].size();
  return 1;
}

extern "C" JXLFILETYPEIO_API int32_t jxlhip_encoder_stage_times(JxlHipEncoder* enc, const char** names, float* ms, int32_t capacity) {
  if (!enc) return 0;
  int32_t k = 0;
  for (auto& e : enc->stages) {
    if (k >= capacity) break;
    if (names) names[k] = e.first;
    if (ms) ms[k] = e.second;
    k++;
  }
  return k;
}
