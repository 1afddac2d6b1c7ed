// Host orchestration of the HIP decode path and the C-ABI (include/jxlfiletypeio.h).
//
// LoadImage mirrors DecoderReadImage (reference: src/JxlFileTypeIO/Decoder/JxlDecoder.cpp:796-852):
// pass 1 = headers + metadata callbacks (:412-793), pass 2 = frame -> one interleaved buffer ->
// setLayerData (:217-410).  The arithmetic that the reference delegates to libjxl
// (JxlDecoderProcessInput, :252) runs in the kernels of kernels.hip.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "../../include/jxlfiletypeio.h"
#include "animation.h"
#include "batch_layout.h"
#include "entropy_plan.h"
#include "host_parse.h"
#include "icc.h"
#include "kernels.h"

namespace jxlhip {

struct HipError : std::runtime_error {
  explicit HipError(const std::string& m) : std::runtime_error(m) {}
};
#define HIP_OK(expr)                                                                                      \
  do {                                                                                                    \
    hipError_t e_ = (expr);                                                                               \
    if (e_ != hipSuccess) throw HipError(std::string(#expr) + ": " + hipGetErrorString(e_));              \
  } while (0)

static void SetErr(ErrorInfo* e, const char* fmt, ...) {
  if (!e) return;
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  int n = vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  // reference semantics (Common.cpp:18-53): only messages of 1..255 chars are stored
  if (n > 0 && n <= 255) memcpy(e->errorMessage, buf, (size_t)n + 1);
  else if (n > 255) { memcpy(e->errorMessage, buf, 255); e->errorMessage[255] = 0; }
}

struct StageTimer {
  std::vector<const char*> names;
  std::vector<hipEvent_t> ev;
};

}  // namespace jxlhip

using namespace jxlhip;

// Experiment knobs (environment variables read by tools/sweep_*.sh) exist only in a library built with -DJXLHIP_EXPERIMENTS
// (JXLHIP_EXTRA_CFLAGS): a host process's environment must not be able to change what the shipping library decodes.
static inline const char* Knob(const char* name) {
#ifdef JXLHIP_EXPERIMENTS
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}
static inline bool PowerOfTwoUpTo64(int v) { return v >= 1 && v <= 64 && (v & (v - 1)) == 0; }
static inline int KnobStride(const char* name, int fallback) {   // lane strides: powers of two in 1..64, anything else is ignored
  const char* e = Knob(name);
  if (!e) return fallback;
  const int v = atoi(e);
  return PowerOfTwoUpTo64(v) ? v : fallback;
}

struct JxlHipDecoder {
  int device = 0;
  hipStream_t own_stream = nullptr;
  // static tables
  float* d_basis_all = nullptr;
  float* d_basis_small = nullptr;
  float* d_basis_mfma = nullptr;   // the 32- and 64-point bases laid out per matrix-core lane (tile_kernels.hip: MfmaChainT)
  float* d_llf_scale = nullptr;
  uint16_t* d_natural[kNumOrders] = {};
  U32x2* d_scan[kNumQuantTables] = {};   // per quant table: {order[k], weight bits} in scan order, 3 channels (natural orders, library tables)
  float* d_dq[kNumQuantTables] = {};
  uint32_t dq_n[kNumQuantTables] = {};
  // Per-batch state lives in one of three slots so that, when the caller does not synchronise between batches, the LF
  // stage of batch k+2 (stream_lf), the HF-coefficient stage of batch k+1 (stream_hf) and the alpha + pixel stages of
  // batch k (main stream) run concurrently: the serial entropy kernels leave most issue slots of the chip idle.
  struct Tap { std::vector<uint8_t> qcoef[3], xyb_idct[3], xyb_filtered[3], noise_rnd[3], noise[3]; };   // (noise: frames with the flag only)
  struct Slot {
    // grow-only buffers
    uint8_t* d_ws = nullptr; size_t ws_cap = 0;        // planes
    uint8_t* d_blob = nullptr; size_t blob_cap = 0;    // tables / descriptors / uploaded bitstreams
    uint8_t* h_blob = nullptr; size_t h_blob_cap = 0;  // pinned mirror of d_blob
    uint32_t* h_status = nullptr; size_t h_status_cap = 0;
    int n = 0;
    std::vector<ParsedFrame> frames;
    // layered images: n counts images of the batch (a layered file has one per frame), nfiles the caller's files; file_of maps an image
    // to its file (empty: one image per file); files keeps the parse of each layered file (the codestream its frames point into)
    int nfiles = 0;
    std::vector<int> file_of;
    std::vector<ParsedFrame> files;
    std::vector<DevImage> imgs;          // host copies (device pointers inside)
    std::vector<int> parse_status;
    std::vector<std::string> parse_msg;
    std::vector<size_t> status_off;      // offset of each image's status words in the workspace
    DevImage* d_imgs = nullptr;
    bool pending = false;
    hipEvent_t lf_done = nullptr, hf_done = nullptr, done = nullptr, uploaded = nullptr;
    std::vector<Tap> taps;
    // timing: two event chains (LF stream, main stream)
    std::vector<std::string> stage_names;
    std::vector<int> stage_chain;
    std::vector<hipEvent_t> events;
    std::vector<float> stage_ms;
  };
  static constexpr int kSlots = 3;
  static constexpr int kPixelChunk = 32;   // frames that share one set of reconstruction / filter planes
  Slot slots[kSlots];
  int cur = 0, last = 0;
  Slot* active = &slots[0];
  hipStream_t stream_lf = nullptr;
  hipStream_t stream_hf = nullptr;
  hipStream_t last_stream = nullptr;
  // cumulative per-stage HIP-event time over every finished batch since the last reset (bench: timed region)
  std::vector<std::string> total_names;
  std::vector<double> total_ms;
  int total_batches = 0;
  std::string sticky_error;             // failure of an older, not yet reported batch
  int sticky_status = 0;
  // options
  // LoadImage's device / pinned result buffers, kept between calls of a thread (a 33 MB hipHostMalloc per call costs milliseconds)
  uint8_t* li_dev = nullptr; uint8_t* li_host = nullptr; size_t li_cap = 0;
  void EnsureLoadImageBuffers(size_t bytes);
  int lane_stride_override = 0;
  int hf_stride_override = 0;   // experiment knob: lane stride of the HF kernel only
  bool debug_taps = false;
  // band-restricted decode (multi-GPU sharding of one frame by group rows): 0 rows = whole frame
  int band_first_row = 0, band_rows = 0;
  bool no_stream_pairs = false;   // every fused frame through the four-pixels-per-lane filter kernel (parity tests: same output either way)
  bool no_lf_pipeline = false;    // every LF channel through lf_finish_kernel's row-per-lane prediction pass (parity tests: same output either way)
  // alpha groups of the lane path whose rows are all gradient rows keep their residuals as int16 between the two alpha phases while
  // |residual| <= this (a group with a larger one is decoded again as int32: same output either way); 0: int32 for all
  int alpha_narrow_limit = 32767;
  int alpha_sample_limit = 255;   // largest sample the one-pass alpha form keeps (lower: ordinary files reach its give-up path)
  bool no_direct = false, mod_lanes64 = false;   // launch shapes of the vector loops for small launches too (parity tests: same output either way)
  bool overlap = true;
  // reduced-size decode: 1 = full size; 8 = every image of the next batches leaves at ceil(w / 8) x ceil(h / 8), one pixel
  // per 8x8 cell (VarDCT: the LF image; Modular: cell means of the full decode)
  int downscale = 1;
  bool single_slot = false;   // every batch in workspace slot 0 (an animation's chunks are synchronous: one workspace, not three)

  explicit JxlHipDecoder(int dev);
  ~JxlHipDecoder();
  void EnsureWs(size_t bytes);
  void EnsureBlob(size_t bytes);
  void Mark(const char* name, hipStream_t s, int chain);
  void WaitSlot(Slot& S);
  static DecoderStatus ImageStatus(const Slot& S, int i);
  static std::string FailureText(const Slot& S, int i);
  void NoteOlderFailure(Slot& S);
  Slot& Last() { return slots[last]; }
  // preparsed (a chunk of an animation, JxlHipAnimation::RunChunk): the parse of the call's one file - a single frame, or a layered file
  // whose Layers carry the chunk's frames; it is moved from, and no host bytes are read.
  void Decode(int32_t n_, const uint8_t* const* host_data, const size_t* sizes, const uint8_t* const* dev_data,
              uint8_t* const* dev_out, hipStream_t stream, bool sync, DecoderStatus* statuses, ErrorInfo* err, ParsedFrame* preparsed = nullptr);
  DecoderStatus Finish(DecoderStatus* statuses, ErrorInfo* err);
  void CopyPlaneTap(int stage);
  void PrepassSingle(ParsedFrame& f, const uint8_t* dev_file);
  EntropyPlanOptions PlanOptions() const;
};

JxlHipDecoder::JxlHipDecoder(int dev) {
  if (dev < 0) HIP_OK(hipGetDevice(&dev));
  device = dev;
  HIP_OK(hipSetDevice(device));
  // (measured on MI355X, batch 384: stream priorities and CU masks that confine the entropy streams to part of the chip change
  // nothing or lose - the three chains already add up to the chip's capacity)
  // JXLHIP_ENTROPY_CUS=N (experiments build): the two entropy streams may only use N of the 256 CUs (the mask's bits go round the
  // XCDs, so N / 8 per XCD); JXLHIP_PIXEL_CUS=M: this object's own stream keeps off the first 256 - M.
  int entropy_cus = 0, pixel_cus = 0;
  if (const char* e = Knob("JXLHIP_ENTROPY_CUS")) entropy_cus = std::min(256, std::max(0, atoi(e)));
  if (const char* e = Knob("JXLHIP_PIXEL_CUS")) pixel_cus = std::min(256, std::max(0, atoi(e)));
  auto masked_stream = [](hipStream_t* s, int first, int count) {
    uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = first; i < first + count; i++) mask[i >> 5] |= 1u << (i & 31);
    HIP_OK(hipExtStreamCreateWithCUMask(s, 8, mask));
  };
  if (pixel_cus) masked_stream(&own_stream, 256 - pixel_cus, pixel_cus);
  else HIP_OK(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
  // The entropy chains are latency-bound (a kernel lasts as long as its longest section) and need few wavefronts, but ALL of them at
  // once: while their workgroups queue behind a pixel kernel's thousands of short ones, an entropy kernel runs in rounds and takes a
  // multiple of its time.  Their streams get the highest priority, so that their workgroups take the next free slots.
  int prio_least = 0, prio_greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  const int prio = Knob("JXLHIP_NO_PRIORITY") ? prio_least : prio_greatest;
  if (entropy_cus) {
    masked_stream(&stream_lf, 0, entropy_cus);
    masked_stream(&stream_hf, 0, entropy_cus);
  } else {
    HIP_OK(hipStreamCreateWithPriority(&stream_lf, hipStreamNonBlocking, prio));
    HIP_OK(hipStreamCreateWithPriority(&stream_hf, hipStreamNonBlocking, prio));
  }
  for (auto& S : slots) {
    HIP_OK(hipEventCreateWithFlags(&S.lf_done, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&S.hf_done, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&S.uploaded, hipEventDisableTiming));
  }
  if (const char* e = Knob("JXLHIP_NO_OVERLAP")) overlap = atoi(e) == 0;
  const StaticTables& st = GetStaticTables();
  std::vector<float> all;
  for (int i = 0; i < 6; i++) all.insert(all.end(), st.basis[i].begin(), st.basis[i].end());
  HIP_OK(hipMalloc(&d_basis_all, all.size() * 4));
  HIP_OK(hipMemcpy(d_basis_all, all.data(), all.size() * 4, hipMemcpyHostToDevice));
  std::vector<float> small;
  for (int c = 1; c <= 32; c *= 2)
    for (int k = 0; k < c; k++)
      for (int nn = 0; nn < c; nn++) small.push_back((float)((k ? std::sqrt(2.0) : 1.0) * std::cos((2 * nn + 1) * k * M_PI / (2.0 * c))));
  {
    // for lane (n, q) of a 16x16x4 product over an N-point transform: basis[(4 k + q) * N + n], k = 0 .. N/4-1, contiguous
    std::vector<float> t;
    for (int li = 2; li <= 3; li++) {   // N = 32, 64  (st.basis[li]: N = 8 << li)
      const int N = 8 << li;
      const std::vector<float>& b = st.basis[li];
      for (int nn = 0; nn < N; nn++)
        for (int q = 0; q < 4; q++)
          for (int k = 0; k < N / 4; k++) t.push_back(b[(size_t)(4 * k + q) * N + nn]);
    }
    HIP_OK(hipMalloc(&d_basis_mfma, t.size() * 4));
    HIP_OK(hipMemcpy(d_basis_mfma, t.data(), t.size() * 4, hipMemcpyHostToDevice));
  }
  HIP_OK(hipMalloc(&d_basis_small, small.size() * 4));
  HIP_OK(hipMemcpy(d_basis_small, small.data(), small.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMalloc(&d_llf_scale, st.llf_scale.size() * 4));
  HIP_OK(hipMemcpy(d_llf_scale, st.llf_scale.data(), st.llf_scale.size() * 4, hipMemcpyHostToDevice));
  for (int o = 0; o < kNumOrders; o++) {
    HIP_OK(hipMalloc(&d_natural[o], st.natural_order[o].size() * 2));
    HIP_OK(hipMemcpy(d_natural[o], st.natural_order[o].data(), st.natural_order[o].size() * 2, hipMemcpyHostToDevice));
  }
  for (int q = 0; q < kNumQuantTables; q++) {
    HIP_OK(hipMalloc(&d_dq[q], st.dq[q].size() * 4));
    HIP_OK(hipMemcpy(d_dq[q], st.dq[q].data(), st.dq[q].size() * 4, hipMemcpyHostToDevice));
    dq_n[q] = (uint32_t)(st.dq[q].size() / 3);
    std::vector<U32x2> sl(3 * (size_t)dq_n[q]);
    BuildScanList(q, nullptr, sl.data());
    HIP_OK(hipMalloc(&d_scan[q], sl.size() * sizeof(U32x2)));
    HIP_OK(hipMemcpy(d_scan[q], sl.data(), sl.size() * sizeof(U32x2), hipMemcpyHostToDevice));
  }
  lane_stride_override = KnobStride("JXLHIP_LANE_STRIDE", 0);
  hf_stride_override = KnobStride("JXLHIP_HF_STRIDE", 0);
}

JxlHipDecoder::~JxlHipDecoder() {
  (void)hipSetDevice(device);
  // batches still in flight read and write the slots' memory and record the slots' events: every pending one is waited for by name
  // (errors ignored: a failed batch is over as well) before anything of its slot goes
  for (auto& S : slots)
    if (S.pending && S.done) { (void)hipEventSynchronize(S.done); S.pending = false; }
  (void)hipDeviceSynchronize();
  for (auto& S : slots) {
    for (auto e : S.events) (void)hipEventDestroy(e);
    if (S.lf_done) (void)hipEventDestroy(S.lf_done);
    if (S.hf_done) (void)hipEventDestroy(S.hf_done);
    if (S.done) (void)hipEventDestroy(S.done);
    if (S.uploaded) (void)hipEventDestroy(S.uploaded);
    (void)hipFree(S.d_ws); (void)hipFree(S.d_blob);
    if (S.h_blob) (void)hipHostFree(S.h_blob);
    if (S.h_status) (void)hipHostFree(S.h_status);
  }
  (void)hipFree(d_basis_all); (void)hipFree(d_basis_small); (void)hipFree(d_basis_mfma); (void)hipFree(d_llf_scale);
  for (auto p : d_natural) (void)hipFree(p);
  for (auto p : d_dq) (void)hipFree(p);
  for (auto p : d_scan) (void)hipFree(p);
  if (li_dev) (void)hipFree(li_dev);
  if (li_host) (void)hipHostFree(li_host);
  if (own_stream) (void)hipStreamDestroy(own_stream);
  if (stream_lf) (void)hipStreamDestroy(stream_lf);
  if (stream_hf) (void)hipStreamDestroy(stream_hf);
}

void JxlHipDecoder::EnsureLoadImageBuffers(size_t bytes) {
  if (bytes <= li_cap) return;
  if (li_dev) { (void)hipFree(li_dev); li_dev = nullptr; }
  if (li_host) { (void)hipHostFree(li_host); li_host = nullptr; }
  li_cap = 0;
  HIP_OK(hipMalloc(&li_dev, bytes));
  HIP_OK(hipHostMalloc(&li_host, bytes, hipHostMallocDefault));
  li_cap = bytes;
}

void JxlHipDecoder::EnsureWs(size_t bytes) {
  auto& d_ws = active->d_ws; auto& ws_cap = active->ws_cap;
  if (bytes <= ws_cap) return;
  if (d_ws) HIP_OK(hipFree(d_ws));
  d_ws = nullptr;
  ws_cap = 0;
  size_t cap = bytes + bytes / 8;
  HIP_OK(hipMalloc(&d_ws, cap));
  ws_cap = cap;
}

void JxlHipDecoder::EnsureBlob(size_t bytes) {
  auto& d_blob = active->d_blob; auto& blob_cap = active->blob_cap; auto& h_blob = active->h_blob; auto& h_blob_cap = active->h_blob_cap;
  if (bytes > blob_cap) {
    if (d_blob) HIP_OK(hipFree(d_blob));
    d_blob = nullptr;
    blob_cap = 0;
    size_t cap = bytes + bytes / 4 + 4096;
    HIP_OK(hipMalloc(&d_blob, cap));
    blob_cap = cap;
  }
  if (bytes > h_blob_cap) {
    if (h_blob) HIP_OK(hipHostFree(h_blob));
    h_blob = nullptr;
    h_blob_cap = 0;
    size_t cap = bytes + bytes / 4 + 4096;
    HIP_OK(hipHostMalloc(&h_blob, cap, hipHostMallocDefault));
    h_blob_cap = cap;
  }
}

void JxlHipDecoder::Mark(const char* name, hipStream_t s, int chain) {
  Slot& S = *active;
  size_t i = S.stage_names.size();
  S.stage_names.push_back(name);
  S.stage_chain.push_back(chain);
  if (S.events.size() <= i) {
    hipEvent_t e;
    HIP_OK(hipEventCreate(&e));
    S.events.push_back(e);
  }
  HIP_OK(hipEventRecord(S.events[i], s));
}

// Waits for a submitted batch and folds a failure into the sticky error (reported by the next Finish).
void JxlHipDecoder::WaitSlot(Slot& S) {
  if (!S.pending) return;
  HIP_OK(hipEventSynchronize(S.done));
  S.pending = false;
  // a stage's time = from the previous mark of ITS chain (stream) to its own; marks of different chains may interleave in the list
  S.stage_ms.assign(S.stage_names.size(), -1.f);
  {
    int last_of[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    for (size_t i = 0; i < S.stage_names.size(); i++) {
      const int c = S.stage_chain[i] & 7;
      if (last_of[c] >= 0) { S.stage_ms[i] = 0.f; (void)hipEventElapsedTime(&S.stage_ms[i], S.events[last_of[c]], S.events[i]); }
      last_of[c] = (int)i;
    }
  }
  for (size_t i = 1; i < S.stage_names.size(); i++) {
    if (S.stage_ms[i] < 0.f) continue;   // the first mark of a chain: a start, not a stage
    size_t k = 0;
    while (k < total_names.size() && total_names[k] != S.stage_names[i]) k++;
    if (k == total_names.size()) { total_names.push_back(S.stage_names[i]); total_ms.push_back(0.0); }
    total_ms[k] += S.stage_ms[i];
  }
  total_batches++;
}

// Status of image i of a finished batch: the host's (parse, refusal) or, for an image that went to the device, what its status words say.
DecoderStatus JxlHipDecoder::ImageStatus(const Slot& S, int i) {
  const DecoderStatus st = (DecoderStatus)S.parse_status[i];
  if (st == DecoderStatus_Ok && S.h_status[(size_t)i * 16]) return DecoderStatus_DecodeError;
  return st;
}

// What went wrong with image i of a finished batch (ImageStatus != Ok): the host's message, or the device's flags, the caller's file
// and the failing sections.  One text for the last batch's error and for the sticky error of an older one.
std::string JxlHipDecoder::FailureText(const Slot& S, int i) {
  if (S.parse_status[i] != DecoderStatus_Ok) return S.parse_msg[i];
  const int file = S.file_of.empty() ? i : S.file_of[i];
  const uint32_t* w = S.h_status + (size_t)i * 16;   // [3..7]: last failing section + 1 of lf_ans / lf_finish / hf_decode / alpha_ans / modular
  const uint32_t bits = w[0];
  char buf[256];
  if (bits & kErrUnsupportedTransform) snprintf(buf, sizeof(buf), "AFV transforms are not supported (image %d, LF group section %u)", file, w[4]);
  else snprintf(buf, sizeof(buf), "GPU decode failed (flags 0x%x:%s%s%s%s%s; image %d, sections lf %u hf %u alpha %u)", bits, bits & kErrBitstream ? " corrupt-bitstream" : "",
                bits & kErrUnsupportedHeader ? " unsupported-modular-header" : "", bits & kErrUnsupportedTree ? " unsupported-tree" : "",
                bits & kErrBlockLayout ? " invalid-varblock-layout" : "", bits & kErrRange ? " value-out-of-range" : "", file, w[3], w[5], w[6]);
  return buf;
}

// The first failure of a finished batch that is not the most recent one becomes the sticky error, unless an older one is already kept.
void JxlHipDecoder::NoteOlderFailure(Slot& S) {
  for (int i = 0; i < S.n && sticky_status == DecoderStatus_Ok; i++) {
    const DecoderStatus st = ImageStatus(S, i);
    if (st != DecoderStatus_Ok) { sticky_status = st; sticky_error = "an earlier asynchronous batch failed: " + FailureText(S, i); }
  }
}

// The entropy plan's options: this object's, and the experiment knobs' values.
EntropyPlanOptions JxlHipDecoder::PlanOptions() const {
  EntropyPlanOptions o;
  o.band_first_row = band_first_row; o.band_rows = band_rows;
  o.downscale = downscale;
  o.lane_stride_override = lane_stride_override; o.hf_stride_override = hf_stride_override;
  o.no_direct = no_direct || Knob("JXLHIP_NO_DIRECT"); o.mod_lanes64 = mod_lanes64 || Knob("JXLHIP_MOD_LANES64");
  o.hf_waves8 = Knob("JXLHIP_HF_WAVES8"); o.alpha_old_shapes = Knob("JXLHIP_ALPHA_OLD_SHAPES"); o.no_hf_sort = Knob("JXLHIP_NO_HF_SORT");
  o.hf_global = Knob("JXLHIP_HF_GLOBAL"); o.alpha_global = Knob("JXLHIP_ALPHA_GLOBAL"); o.lf_global = Knob("JXLHIP_LF_GLOBAL");
  if (const char* e = Knob("JXLHIP_HF_LDS_KB")) o.hf_lds_kb = atoi(e);
  o.alpha_stride = KnobStride("JXLHIP_ALPHA_STRIDE", 0);
  if (const char* e = Knob("JXLHIP_LF_PER_WAVE")) o.lf_per_wave = std::max(1, atoi(e));
  return o;
}

void JxlHipDecoder::Decode(int32_t n_, const uint8_t* const* host_data, const size_t* sizes, const uint8_t* const* dev_data,
                           uint8_t* const* dev_out, hipStream_t stream, bool sync, DecoderStatus* statuses, ErrorInfo* err, ParsedFrame* preparsed) {
  HIP_OK(hipSetDevice(device));
  if (!stream) stream = own_stream;
  Slot& S = slots[cur];
  active = &S;
  if (S.pending) {
    // the slot is reused: its previous batch must be complete; remember a failure nobody has looked at yet
    WaitSlot(S);
    NoteOlderFailure(S);
  }
  auto& d_ws = S.d_ws; auto& d_blob = S.d_blob; auto& h_blob = S.h_blob; auto& h_status = S.h_status; auto& h_status_cap = S.h_status_cap;
  auto& n = S.n; auto& frames = S.frames; auto& imgs = S.imgs; auto& parse_status = S.parse_status; auto& parse_msg = S.parse_msg;
  auto& status_off = S.status_off; auto& d_imgs = S.d_imgs; auto& taps = S.taps; auto& stage_names = S.stage_names;
  hipStream_t s_lf = (overlap && !debug_taps) ? stream_lf : stream;
  hipStream_t s_hf = (overlap && !debug_taps) ? stream_hf : stream;
  n = n_;
  frames.assign(n, ParsedFrame());
  parse_status.assign(n, DecoderStatus_Ok);
  parse_msg.assign(n, "");
  // ---- 1. host parse (threaded across images)
  if (preparsed) {
    frames[0] = std::move(*preparsed);
  } else {
    int nt = std::min<int>(n, std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
    std::vector<std::thread> th;
    std::atomic<int> next(0);
    auto work = [&]() {
      for (;;) {
        int i = next.fetch_add(1);
        if (i >= n) return;
        try {
          ParseFile(host_data[i], sizes[i], false, frames[i]);
        } catch (const ParseError& e) {
          parse_status[i] = e.status;
          parse_msg[i] = e.what();
        } catch (const std::bad_alloc&) {
          parse_status[i] = DecoderStatus_OutOfMemory;
        } catch (const std::exception& e) {
          parse_status[i] = DecoderStatus_DecodeError;
          parse_msg[i] = e.what();
        }
      }
    };
    if (nt <= 1) work();
    else {
      for (int t = 0; t < nt; t++) th.emplace_back(work);
      for (auto& t : th) t.join();
    }
  }
  // ---- layered images: every frame up to the displayed one becomes an image of the batch, decoded like any other into f32 scratch;
  // compose_kernel blends them onto the canvas at the end.  Status words stay per image; Finish folds them per file.
  S.nfiles = n;
  S.file_of.clear();
  S.files.clear();
  std::vector<Composite> comps;
  std::vector<const uint8_t*> x_dev_data;
  std::vector<uint8_t*> x_dev_out;
  // reduced-size decode: what it does not cover is refused per image, before anything is laid out or launched for it (crop origins and
  // patch positions are no multiples of 8; a band is a set of full-size pixel rows)
  const bool ds = downscale == 8;
  if (ds)
    for (int i = 0; i < n; i++) {
      if (parse_status[i] != DecoderStatus_Ok) continue;
      const char* why = nullptr;
      if (band_rows > 0) why = "downscale 8: band decode is not supported";
      else if (frames[i].layers) why = frames[i].layers->patches ? "downscale 8: images with patches are not supported" : "downscale 8: layered images are not supported";
      if (why) { parse_status[i] = DecoderStatus_DecodeError; parse_msg[i] = why; }
    }
  for (int i = 0; i < n; i++)
    if (parse_status[i] == DecoderStatus_Ok && frames[i].layers && band_rows > 0) {
      parse_status[i] = DecoderStatus_DecodeError;
      parse_msg[i] = frames[i].layers->patches ? "band decode of an image with patches is not supported" : "band decode of a layered image is not supported";
    }
  bool any_layered = false;
  for (int i = 0; i < n; i++) any_layered |= parse_status[i] == DecoderStatus_Ok && frames[i].layers != nullptr;
  if (any_layered) {
    std::vector<ParsedFrame> xf;
    std::vector<int> xst;
    std::vector<std::string> xmsg;
    S.files.reserve(n);
    for (int i = 0; i < n; i++) {
      if (parse_status[i] == DecoderStatus_Ok && frames[i].layers) {
        std::shared_ptr<Layers> lay = frames[i].layers;
        comps.push_back(Composite{i, (int)xf.size(), (int)lay->frames.size(), lay->save, dev_out[i]});
        for (auto& fr : lay->frames) {
          fr.orientation = 1;   // frames stay in codestream orientation; the compositor orients the displayed image
          xf.push_back(std::move(fr));
          xst.push_back(DecoderStatus_Ok);
          xmsg.emplace_back();
          S.file_of.push_back(i);
          x_dev_data.push_back(dev_data ? dev_data[i] : nullptr);
          x_dev_out.push_back(nullptr);
        }
        S.files.push_back(std::move(frames[i]));
        continue;
      }
      xf.push_back(std::move(frames[i]));
      xst.push_back(parse_status[i]);
      xmsg.push_back(parse_msg[i]);
      S.file_of.push_back(i);
      x_dev_data.push_back(dev_data ? dev_data[i] : nullptr);
      x_dev_out.push_back(dev_out[i]);
    }
    frames.swap(xf);
    parse_status.swap(xst);
    parse_msg.swap(xmsg);
    n = (int)frames.size();
    if (dev_data) dev_data = x_dev_data.data();
    dev_out = x_dev_out.data();
  }
  // frames that fit one group: their HfGlobal can only be located once the LF group has been decoded (one bit stream)
  for (int i = 0; i < n; i++) {
    if (parse_status[i] != DecoderStatus_Ok || !frames[i].single || frames[i].encoding != 0) continue;
    try {
      PrepassSingle(frames[i], dev_data ? dev_data[i] : nullptr);
    } catch (const ParseError& e) {
      parse_status[i] = e.status;
      parse_msg[i] = e.what();
    } catch (const std::exception& e) {
      parse_status[i] = DecoderStatus_DecodeError;
      parse_msg[i] = e.what();
    }
  }
  // A band is a set of VarDCT group rows.  A Modular frame has no band mode (global Squeeze / whole-image transforms: SURVEY 8e
  // "replicas only"); its output kernel writes the whole frame, so accepting the option would overrun the caller's band buffer.
  for (int i = 0; i < n; i++)
    if (parse_status[i] == DecoderStatus_Ok && band_rows > 0 && (band_first_row < 0 || band_first_row >= (int)frames[i].yg)) {
      parse_status[i] = DecoderStatus_DecodeError;
      parse_msg[i] = "band decode: the first group row lies outside the frame";
    }
  for (int i = 0; i < n; i++)
    if (parse_status[i] == DecoderStatus_Ok && band_rows > 0 && frames[i].encoding == 1) {
      parse_status[i] = DecoderStatus_DecodeError;
      parse_msg[i] = "band decode of a Modular (lossless) frame is not supported";
    }
  for (int i = 0; i < n; i++)
    if (parse_status[i] == DecoderStatus_Ok && band_rows > 0 && frames[i].orientation != 1) {
      parse_status[i] = DecoderStatus_DecodeError;
      parse_msg[i] = "band decode of a frame with an orientation is not supported";
    }
  // images that failed to parse or were refused are skipped on the device (their DevImage stays zeroed, ng = 0)
  // ---- 2. the entropy stage's plan (entropy_plan.h): decoded ranges, lane mappings, task tables, LDS sizes
  const EntropyPlan plan = PlanEntropy(frames, parse_status, PlanOptions());
  // ---- 3. layout of blob and workspace (batch_layout.h): one pass measures, the same code then places
  const PatchTables patches = comps.empty() ? PatchTables() : BuildPatchTables(frames, parse_status, comps);
  BatchInput in;
  in.frames = &frames; in.parse_status = &parse_status; in.plan = &plan;
  in.dev_data = dev_data; in.dev_out = dev_out;
  in.comps = &comps; in.patches = &patches; in.file_of = &S.file_of; in.files = &S.files; in.nfiles = S.nfiles;
  in.d_natural = d_natural; in.d_scan = d_scan; in.d_dq = d_dq; in.dq_n = dq_n;
  in.ds = ds; in.debug_taps = debug_taps; in.no_stream_pairs = no_stream_pairs; in.pixel_chunk_cap = kPixelChunk;
  BatchRegions measured;
  {
    BatchOutput unplaced;
    BuildBatch(in, measured, unplaced);
  }
  const size_t blob_bytes = measured.blob.off, zero_bytes = measured.ZeroBytes();
  EnsureBlob(blob_bytes);
  EnsureWs(measured.WorkspaceBytes());
  if ((size_t)n * 16 > h_status_cap) {
    if (h_status) HIP_OK(hipHostFree(h_status));
    h_status = nullptr;
    HIP_OK(hipHostMalloc(&h_status, (size_t)n * 16 * 4 + 64, hipHostMallocDefault));
    h_status_cap = (size_t)n * 16;
  }
  // ---- 4. fill the pinned blob
  memset(h_blob, 0, blob_bytes);
  BatchRegions placed{Region(h_blob, d_blob, blob_bytes), Region(nullptr, d_ws, measured.zero.off), Region(nullptr, d_ws + zero_bytes, measured.ws.off),
                      Region(nullptr, d_ws + measured.PixStart(), measured.pix.off)};
  BatchOutput B;
  BuildBatch(in, placed, B);
  imgs.swap(B.imgs);
  status_off.swap(B.status_off);
  d_imgs = B.d_imgs;
  const bool any_alpha = B.any_alpha, any_noise = B.any_noise;
  const int pixel_chunk = B.pixel_chunk, max_groups = B.max_groups;
  const int nlf_t = (int)plan.lf_finish_tasks.size(), npass_t = (int)plan.pass_tasks.size(), nalpha_t = (int)plan.alpha_tasks.size();
  const int nlf_ans_t = (int)plan.lf_ans_tasks.size(), nmod_t = (int)plan.mod_tasks.size();
  if (Knob("JXLHIP_DEBUG_LDS")) {
    for (int i = 0; i < std::min(n, 8); i++)
      if (parse_status[i] == DecoderStatus_Ok && frames[i].encoding == 0)
        fprintf(stderr, "[jxlhip] image %d: hf tables %zu B (clusters %u, log_alpha %u, contexts %zu), lanes/wg %d; modular tables: clusters %u log_alpha %u contexts %zu tree %zu\n", i,
                plan.frames[i].hf_table_bytes, frames[i].acode.num_hist, frames[i].acode.log_alpha, frames[i].acode.ctx_map.size(), plan.frames[i].hf_per_wg,
                frames[i].mcode.num_hist, frames[i].mcode.log_alpha, frames[i].mcode.ctx_map.size(), frames[i].tree.size());
    fprintf(stderr, "[jxlhip] launch LDS: hf %zu B (lanes %zu), lf %zu B, alpha %zu B; hf workgroups %d x %d threads, stride %d; alpha workgroups %d; lf_ans workgroups %d\n",
            plan.hf.lds, plan.lds_hf_lanes, plan.lf.lds, plan.alpha.lds, npass_t, plan.hf_waves * 64, plan.lane_stride, nalpha_t, nlf_ans_t);
  }
  // ---- 5. enqueue: LF chain on s_lf, everything that needs the block layout on the main stream
  stage_names.clear();
  S.stage_chain.clear();
  Mark("start", s_lf, 0);
  // experiment knob (timing only, the output is stale): bit 0 skips the LF chain, 1 the HF decode, 2 alpha, 3 reconstruction, 4 filters -
  // with the same files resubmitted, a skipped stage's results of the previous batch in this workspace slot are still in place
  static const int skip_stages = Knob("JXLHIP_SKIP_STAGES") ? atoi(Knob("JXLHIP_SKIP_STAGES")) : 0;
  if (!(skip_stages & 1)) HIP_OK(hipMemsetAsync(d_ws, 0, zero_bytes, s_lf));
  HIP_OK(hipMemcpyAsync(d_blob, h_blob, blob_bytes, hipMemcpyHostToDevice, s_lf));
  Mark("upload+clear", s_lf, 0);
  // Synthetic noise depends on nothing but the uploaded descriptors: the first pixel chunk's planes are generated and convolved on the
  // main stream while the entropy chains run on theirs (a group's generator is a chain of 12 288 dependent steps, 1.25 ms for a 4K
  // frame).  The random planes borrow the chunk's tmp planes and are dead again before the reconstruction needs those.  Later chunks
  // share the first one's planes and wait their turn in the pixel loop; so does everything when one stream carries the whole decode.
  const bool pix_on_hf = Knob("JXLHIP_PIX_ON_HF") && s_hf != stream;
  const bool early_noise = any_noise && !debug_taps && s_lf != stream && !pix_on_hf;
  if (early_noise) {
    HIP_OK(hipEventRecord(S.uploaded, s_lf));
    HIP_OK(hipStreamWaitEvent(stream, S.uploaded, 0));
    Mark("noise_start", stream, 3);
    LaunchNoise(d_imgs, std::min(pixel_chunk, n), max_groups, B.max_w, B.max_h, stream);
    Mark("noise", stream, 3);
  }
  if (!(skip_stages & 1)) {
  LaunchLfAns(d_imgs, B.lf_ans_tasks, nlf_ans_t, plan.lf_per_wave, plan.lf.Bytes(), plan.direct_lf, plan.lean_mod, s_lf);
  Mark("lf_ans", s_lf, 0);
  LaunchLfFinish(d_imgs, B.lf_tasks, nlf_t, !no_lf_pipeline, s_lf);
  if (!ds || any_alpha) LaunchHfBlockList(d_imgs, n, max_groups, s_lf);   // (the varblock lists serve hf_decode_kernel alone)
  LaunchLfPixelStages(d_imgs, n, B.max_cells, s_lf);
  }
  Mark("lf_finish+pixels", s_lf, 0);
  // three chains, three streams: LF (batch k+2) | HF coefficients (batch k+1) | alpha + pixels (batch k)
  if (s_lf != s_hf) {
    HIP_OK(hipEventRecord(S.lf_done, s_lf));
    HIP_OK(hipStreamWaitEvent(s_hf, S.lf_done, 0));
  }
#ifdef JXLHIP_EXPERIMENTS
  // JXLHIP_INTERFERE=kind,workgroups-per-CU,LDS-KB,ms: a probe kernel that occupies one resource (kernels.hip) starts with the HF stage on a
  // stream of its own and runs for `ms`: which stage is sensitive to which resource (tools/interfere.sh)
  if (const char* e = Knob("JXLHIP_INTERFERE")) {
    int kind = 0, wgs = 1, lds_kb = 64; float ms = 100.f;
    if (sscanf(e, "%d,%d,%d,%f", &kind, &wgs, &lds_kb, &ms) >= 1 && kind >= 1 && kind <= 6 && wgs >= 1 && wgs <= 16 && lds_kb >= 1 && lds_kb <= 160 && ms > 0 && ms < 2000) {
      static hipStream_t xs = nullptr;
      static float* xbuf = nullptr;
      const size_t xbytes = (size_t)512 << 20;
      if (!xs) { HIP_OK(hipStreamCreateWithFlags(&xs, hipStreamNonBlocking)); HIP_OK(hipMalloc(&xbuf, xbytes)); }
      if (s_lf != s_hf) HIP_OK(hipStreamWaitEvent(xs, S.lf_done, 0));
      LaunchInterference(kind, wgs, lds_kb, ms, xbuf, xbytes, xs);
    }
  }
#endif
  Mark("hf_start", s_hf, 1);
  // alpha in one pass belongs to the lane path (several sections per wavefront); one-section launches keep the scalar row loop and two passes
  const int alpha_narrow = plan.direct_alpha ? 0 : alpha_narrow_limit;
  // Reduced-size decode: the HF tokens are read only to find what follows them in a pass-group section, i.e. for frames with alpha
  // (their pass tasks are the only ones listed); stages that do not run leave no entry in the stage times.
  if (!(skip_stages & 2) && (!ds || npass_t))
  LaunchHfDecode(d_imgs, B.pass_tasks, npass_t, plan.hf_waves * 64, plan.lane_stride, plan.hf.Bytes(), plan.lds_hf_lanes, s_hf);
  if (!ds || npass_t) Mark("hf_decode", s_hf, 1);
  // alpha follows the HF tokens in every pass-group section (its first bit is where the HF kernel stopped reading): same chain,
  // necessarily; the main stream carries nothing but the pixel stages
  if (any_alpha && !(skip_stages & 4))
    LaunchAlphaAns(d_imgs, B.alpha_tasks, nalpha_t, plan.alpha_stride, plan.alpha.Bytes(), plan.direct_alpha, plan.lean_mod,
                   alpha_narrow, alpha_sample_limit, s_hf);
  if (!ds || any_alpha) Mark("alpha_ans", s_hf, 1);
  if (debug_taps && !ds) {   // the quantised coefficients as dense planes (every frame has its own planes in this mode)
    taps.assign(n, Tap());
    LaunchExpandCoefficients(d_imgs, n, true, B.max_tiles, stream);
    HIP_OK(hipStreamSynchronize(stream));
    CopyPlaneTap(0);
  }
  // the alpha planes' prediction pass: behind the token pass on the HF stream (the pixel stream is the longest of the three chains
  // since the reconstruction workgroup grew to 72 KB of LDS and the HF kernel keeps its residency beside it: 107.2 against 108.7 ms;
  // while the HF stream was the longest it was the other way round - knob JXLHIP_ALPHA_FINISH_ON_PIX)
  const bool finish_on_hf = s_hf == stream || debug_taps || !Knob("JXLHIP_ALPHA_FINISH_ON_PIX");
  if (finish_on_hf) {
    if (any_alpha && !(skip_stages & 4)) LaunchAlphaFinish(d_imgs, n, max_groups, s_hf);
    if (!ds || any_alpha) Mark("alpha_finish", s_hf, 1);
  }
  if (s_hf != stream) {
    HIP_OK(hipEventRecord(S.hf_done, s_hf));
    HIP_OK(hipStreamWaitEvent(stream, S.hf_done, 0));
  }
  Mark("main_start", stream, 2);
  if (!finish_on_hf) {
    if (any_alpha && !(skip_stages & 4)) LaunchAlphaFinish(d_imgs, n, max_groups, stream);
    Mark("alpha_finish", stream, 2);
  }
  // experiment knob: the pixel stages behind the HF chain on ITS stream (no overlap between a batch's pixels and the next batch's HF decode)
  hipStream_t s_pix = pix_on_hf ? s_hf : stream;
  // every entropy stage of the batch is behind this point on the pixel stream: what they refused is taken out of the output kernels
  if (B.any_vardct) LaunchSkipFailedImages(d_imgs, n, s_pix);
  if (ds && B.any_vardct) {
    // the whole pixel stage of a reduced-size decode: no reconstruction, no noise, no filters, and every image in one launch
    if (any_alpha) LaunchAlphaReduce(d_imgs, n, B.max_ds_cells, s_pix);
    LaunchLfOutput(d_imgs, n, B.max_ds_cells, s_pix);
    Mark("lf_output", s_pix, 2);
  }
  for (int c0 = 0; c0 < (ds ? 0 : n); c0 += pixel_chunk) {
    const int cnt = std::min(pixel_chunk, n - c0);
    if (!(skip_stages & 8))
    LaunchReconTiles(d_imgs + c0, cnt, B.max_tiles, d_basis_all, d_basis_small, d_llf_scale, d_basis_mfma, s_pix);
    Mark("reconstruct", s_pix, 2);   // exactly recon_tile_kernel; one mark per chunk, the per-stage totals add them up
    LaunchExpandCoefficients(d_imgs + c0, cnt, false, B.max_tiles, s_pix);
    LaunchGenericReconstruct(d_imgs + c0, cnt, d_basis_all, d_basis_small, d_llf_scale, s_pix);
    Mark("reconstruct_generic", s_pix, 2);
    if (debug_taps) { HIP_OK(hipStreamSynchronize(s_pix)); CopyPlaneTap(1); }
    // synthetic noise: the random planes go into the tmp planes, which the reconstruction above no longer needs
    if (any_noise && !(early_noise && c0 == 0)) { LaunchNoise(d_imgs + c0, cnt, max_groups, B.max_w, B.max_h, s_pix); Mark("noise", s_pix, 2); }
    if (!(skip_stages & 16))
    LaunchFilterTiles(d_imgs + c0, cnt, B.max_w, B.max_h, B.stage_mask, B.any_unfiltered, B.any_fused, B.any_fused2, s_pix);
    Mark("filters+output", s_pix, 2);
  }
  if (s_pix != stream) {
    HIP_OK(hipEventRecord(S.hf_done, s_pix));
    HIP_OK(hipStreamWaitEvent(stream, S.hf_done, 0));
  }
  if (nmod_t) {
    // Modular (lossless) frames of the batch; they depend on nothing but the upload
    if (s_lf != stream) { HIP_OK(hipEventRecord(S.lf_done, s_lf)); HIP_OK(hipStreamWaitEvent(stream, S.lf_done, 0)); }
    LaunchModularAns(d_imgs, n, B.mod_tasks, nmod_t, plan.mod.Bytes(), plan.max_mod_groups,
                     plan.max_mod_coded, plan.mod_lanes, plan.mod_rb, plan.mod_wp_lds, plan.direct_mod, stream);
    for (auto& op : B.mod_ops) {
      if (op.kind == 3) LaunchModularPalette(op.a, op.b, op.out, op.nout, op.type, op.rw, op.rh, op.status, stream);   // a: palette, b: indices (rw x rh)
      else LaunchModularOp(op.kind, op.a, op.b, op.c, op.aw, op.ah, op.rw, op.rh, op.type, stream);
    }
    LaunchModularOut(d_imgs, n, B.max_mod_pixels, stream);
    if (ds) LaunchBoxReduce(d_imgs, n, B.max_ds_cells, stream);
    Mark("modular", stream, 2);
  }
  if (!patches.tiles.empty()) {
    // patched frames (Modular, f32) are final once modular_out_kernel has run; the compositor reads them next, on the same stream
    LaunchPatches(B.patch_frames, B.patch_tiles, (int)patches.tiles.size(), B.patch_list, B.patch_pos, B.patch_refs, stream);
    Mark("patches", stream, 2);
  }
  if (!comps.empty()) {
    if (B.compose_reduce) LaunchComposeReduce(B.comp_imgs, B.comp_frames, (int)comps.size(), B.max_reduce_cells, stream);
    else LaunchCompose(B.comp_imgs, B.comp_frames, (int)comps.size(), B.max_segments, stream);
    Mark("compose", stream, 2);
  }
  for (int i = 0; i < n; i++)
    if (parse_status[i] == DecoderStatus_Ok && frames[i].orientation != 1 && !ds) {
      const ParsedFrame& f = frames[i];
      LaunchOrient(imgs[i].out, dev_out[i], (int)f.xsize, (int)f.ysize, (int)(OutSamplesPerPixel(f) * OutBytesPerSample(f)), (int)f.orientation, stream);
    }
  LaunchStatusToHost(B.status_base, h_status, n * 16, stream);   // (images that failed to parse: zeros)
  HIP_OK(hipEventRecord(S.done, stream));
  HIP_OK(hipGetLastError());
  last_stream = stream;
  S.pending = true;
  last = cur;
  cur = single_slot ? cur : (cur + 1) % kSlots;
  if (sync) {
    DecoderStatus st = Finish(statuses, err);
    (void)st;
    if (debug_taps && !ds) CopyPlaneTap(2);
  } else if (statuses) {
    for (int i = 0; i < S.nfiles; i++) statuses[i] = DecoderStatus_Ok;
    for (int i = n - 1; i >= 0; i--) {   // a file's first failing image wins
      const int file = S.file_of.empty() ? i : S.file_of[i];
      if (parse_status[i] != DecoderStatus_Ok) statuses[file] = parse_status[i];
    }
  }
}

// LF stage of ONE single-section frame on temporary buffers, synchronously: yields the bit position where HfGlobal starts,
// which the host then parses (ParseHfGlobalAt).  The main pass decodes the (tiny) LF group again with everything in place.
void JxlHipDecoder::PrepassSingle(ParsedFrame& f, const uint8_t* dev_file) {
  // One temporary holds the uploaded tables and, from the next 256 bytes on, what the kernel expects cleared and then scratch; laid out
  // like a batch (batch_layout.h): measured, allocated, placed.  The host writes the first region only, whose staging buffer is as
  // large as that region.
  struct Pre { const DevImage* img; const SectionTask* task; uint32_t* status; uint64_t* lf_end; size_t zero_end; };
  auto lay_out = [&](Region& up, Region& r) {
    Pre p;
    DevImage im;
    memset(&im, 0, sizeof(im));
    im.w = f.xsize; im.h = f.ysize; im.w8 = f.w8; im.h8 = f.h8; im.xlf = im.ylf = im.nlf = 1; im.xg = im.yg = im.ng = 1;
    im.has_alpha = f.alpha_index >= 0;
    im.single = 1; im.alpha_in_global = im.has_alpha;
    im.lf_start_bits = f.after_lf_global_bits;
    p.img = up.Array<DevImage>(1);
    const SectionTask task{0, 0, 1, 0};
    p.task = up.Put(&task, 1);
    im.sec_off = up.Put(f.sec_off.data(), f.sec_off.size());
    im.sec_size = up.Put(f.sec_size.data(), f.sec_size.size());
    im.tree = up.Put(f.tree.data(), f.tree.size()); im.tree_size = (int32_t)f.tree.size();
    PackCode(f.mcode, up, im.mcode);
    im.cs = (dev_file && f.cs_contiguous) ? dev_file + f.cs_file_offset : up.Put(f.cs, f.cs_size, f.cs_size + 16);
    im.cs_size = f.cs_size;
    im.status = p.status = r.Array<uint32_t>(16); im.lf_end_bits = p.lf_end = r.Array<uint64_t>(1); im.lf_count = r.Array<uint32_t>(1);
    im.lf_extra = r.Array<uint8_t>(4); im.lf_desc = r.Array<ChanDesc>(8); im.alpha_desc = r.Array<ChanDesc>(1);
    p.zero_end = r.off;
    for (int c = 0; c < 3; c++) im.lfq[c] = r.Array<int32_t>((size_t)f.w8 * f.h8);
    im.binfo = r.Array<int32_t>(kBinfoInts);
    im.alpha32 = r.Array<int32_t>((size_t)f.xsize * f.ysize);
    if (f.tree_uses_wp) im.wp_lf = r.Array<int32_t>(kWpLfInts);
    if (f.mcode.lz77) im.lz_lf = r.Array<uint32_t>((size_t)1 << 20);   // the LF group's LZ77 window
    if (DevImage* h = up.Host(p.img)) *h = im;
    return p;
  };
  Region m_up, m_rest;
  lay_out(m_up, m_rest);
  const size_t upload = m_up.off, rest_at = Align(upload, 256);
  uint8_t* d = nullptr;
  HIP_OK(hipMalloc(&d, rest_at + m_rest.off));
  std::vector<uint8_t> h(upload, 0);
  Region up(h.data(), d, upload), rest(nullptr, d + rest_at, m_rest.off);
  const Pre p = lay_out(up, rest);
  hipError_t e = hipMemcpy(d, h.data(), upload, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d + rest_at, 0, p.zero_end);
  uint32_t st_words[16] = {0};
  uint64_t lf_end = 0;
  if (e == hipSuccess) {
    const size_t lds = SlotsLdsBytes(64, f.tree.size(), ShapeOf(f.mcode));
    LaunchLfAns(p.img, p.task, 1, 64, lds <= kLdsMax ? lds : 0, 0, false, own_stream);
    e = hipStreamSynchronize(own_stream);
  }
  if (e == hipSuccess) e = hipMemcpy(st_words, p.status, 64, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(&lf_end, p.lf_end, 8, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) throw HipError(std::string("single-group LF pre-pass: ") + hipGetErrorString(e));
  if (st_words[0]) throw ParseError(DecoderStatus_DecodeError, "GPU decode failed in the LF group of a single-group frame (corrupt bitstream)");
  f.hf_start_bits = ParseHfGlobalAt(f, lf_end);
}

void JxlHipDecoder::CopyPlaneTap(int stage) {
  Slot& S = *active;
  auto& n = S.n; auto& parse_status = S.parse_status; auto& imgs = S.imgs; auto& taps = S.taps;
  for (int i = 0; i < n; i++) {
    if (parse_status[i] != DecoderStatus_Ok) continue;
    const DevImage& d = imgs[i];
    size_t bytes = (size_t)d.wp * d.hp * 4;
    for (int c = 0; c < 3; c++) {
      std::vector<uint8_t>& dst = stage == 0 ? taps[i].qcoef[c] : (stage == 1 ? taps[i].xyb_idct[c] : taps[i].xyb_filtered[c]);
      const void* src = stage == 0 ? (const void*)d.coef[c] : (stage == 1 ? (const void*)d.xyb[c] : (const void*)d.stage_in[4][c]);
      dst.resize(bytes);
      HIP_OK(hipMemcpy(dst.data(), src, bytes, hipMemcpyDeviceToHost));
    }
    if (stage == 2 && d.has_noise) {   // w x h, tight rows; rows outside a band's reach are not generated (random planes) / convolved
      const size_t nb = (size_t)d.w * d.h * 4;
      for (int c = 0; c < 3; c++) {
        taps[i].noise_rnd[c].resize(nb); taps[i].noise[c].resize(nb);
        HIP_OK(hipMemcpy(taps[i].noise_rnd[c].data(), d.noise_rnd[c], nb, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(taps[i].noise[c].data(), d.noise[c], nb, hipMemcpyDeviceToHost));
      }
    }
  }
}

DecoderStatus JxlHipDecoder::Finish(DecoderStatus* statuses, ErrorInfo* err) {
  HIP_OK(hipSetDevice(device));
  // older batches first, in submission order (a failure there becomes the sticky error), then the most recent one
  for (int k = 1; k < kSlots; k++) {
    Slot& O = slots[(last + k) % kSlots];
    if (!O.pending) continue;
    WaitSlot(O);
    NoteOlderFailure(O);
  }
  Slot& S = Last();
  WaitSlot(S);
  DecoderStatus worst = DecoderStatus_Ok;
  // statuses and messages are per file: the frames of a layered file are images of their own here, and any failing one fails the file
  std::vector<DecoderStatus> file_st((size_t)S.nfiles, DecoderStatus_Ok);
  for (int i = 0; i < S.n; i++) {
    const int file = S.file_of.empty() ? i : S.file_of[i];
    const DecoderStatus st = ImageStatus(S, i);
    if (st != DecoderStatus_Ok && worst == DecoderStatus_Ok) SetErr(err, "%s", FailureText(S, i).c_str());
    if (st != DecoderStatus_Ok && file_st[file] == DecoderStatus_Ok) file_st[file] = st;
    if (st != DecoderStatus_Ok && worst == DecoderStatus_Ok) worst = st;
  }
  if (statuses) for (int f = 0; f < S.nfiles; f++) statuses[f] = file_st[f];
  if (worst == DecoderStatus_Ok && sticky_status != DecoderStatus_Ok) {
    worst = sticky_status;
    SetErr(err, "%s", sticky_error.c_str());
  }
  sticky_status = DecoderStatus_Ok;
  sticky_error.clear();
  return worst;
}

// ====================================================================== C-ABI
extern "C" {

uint32_t GetLibJxlVersion(void) {
  // This library is not libjxl; it reports the libjxl API level whose behaviour it follows (0.11.1).
  return (0u << 24) | (11u << 16) | (1u << 8);
}

JxlHipDecoder* jxlhip_decoder_create(int32_t device, ErrorInfo* err) {
  try {
    return new JxlHipDecoder(device);
  } catch (const std::exception& e) {
    SetErr(err, "%s", e.what());
    return nullptr;
  }
}

void jxlhip_decoder_destroy(JxlHipDecoder* dec) { delete dec; }

DecoderStatus jxlhip_peek(const uint8_t* data, size_t size, JxlHipImageInfo* info, ErrorInfo* err) {
  if (!data || !info) return DecoderStatus_NullParameter;
  try {
    ParsedFrame f;
    ParseFile(data, size, true, f);
    info->width = f.orientation >= 5 ? f.ysize : f.xsize; info->height = f.orientation >= 5 ? f.xsize : f.ysize;   // as displayed
    info->has_alpha = f.alpha_index >= 0;
    info->num_channels = f.ncolor + (f.black_index >= 0 ? 1 : 0) + info->has_alpha;
    info->bytes_per_sample = (int32_t)OutBytesPerSample(f);
    info->reserved = f.exp_bits ? 1 : 0;   // float samples
    info->xsize_blocks = f.w8; info->ysize_blocks = f.h8;
    info->num_groups = f.ng; info->num_lf_groups = f.nlf;
    info->epf_iters = f.epf_iters; info->gaborish = f.gab;
    info->codestream_bytes = f.cs_size;
    return DecoderStatus_Ok;
  } catch (const ParseError& e) {
    SetErr(err, "%s", e.what());
    return e.status;
  } catch (const std::exception& e) {
    SetErr(err, "%s", e.what());
    return DecoderStatus_DecodeError;
  }
}

DecoderStatus jxlhip_decode_batch(JxlHipDecoder* dec, int32_t n, const uint8_t* const* host_data, const size_t* sizes,
                                  const uint8_t* const* dev_data, uint8_t* const* dev_out, void* stream, int32_t synchronize,
                                  DecoderStatus* statuses, ErrorInfo* err) {
  if (!dec || !host_data || !sizes || !dev_out || n <= 0) return DecoderStatus_NullParameter;
  try {
    dec->Decode(n, host_data, sizes, dev_data, dev_out, (hipStream_t)stream, synchronize != 0, statuses, err);
    if (statuses) for (int i = 0; i < n; i++) if (statuses[i] != DecoderStatus_Ok) return statuses[i];
    return DecoderStatus_Ok;
  } catch (const std::bad_alloc&) {
    return DecoderStatus_OutOfMemory;
  } catch (const std::exception& e) {
    SetErr(err, "%s", e.what());
    return DecoderStatus_DecodeError;
  }
}

DecoderStatus jxlhip_finish(JxlHipDecoder* dec, DecoderStatus* statuses, ErrorInfo* err) {
  if (!dec) return DecoderStatus_NullParameter;
  try {
    return dec->Finish(statuses, err);
  } catch (const std::exception& e) {
    SetErr(err, "%s", e.what());
    return DecoderStatus_DecodeError;
  }
}

int32_t jxlhip_set_option(JxlHipDecoder* dec, const char* name, int32_t value) {
  if (!dec || !name) return 0;
  if (!strcmp(name, "debug_taps")) { dec->debug_taps = value != 0; return 1; }
  if (!strcmp(name, "query_pixel_chunk")) return JxlHipDecoder::kPixelChunk;
  // values a kernel's indexing depends on are validated here: a negative band start would put pixel rows in front of the caller's
  // band buffer, a stride that is not a power of two breaks the section -> lane mapping
  if (!strcmp(name, "lane_stride")) { if (value != 0 && !PowerOfTwoUpTo64(value)) return 0; dec->lane_stride_override = value; return 1; }
  if (!strcmp(name, "band_first_row")) { if (value < 0) return 0; dec->band_first_row = value; return 1; }
  if (!strcmp(name, "band_rows")) { if (value < 0) return 0; dec->band_rows = value; return 1; }
  if (!strcmp(name, "no_direct")) { dec->no_direct = value != 0; return 1; }
  if (!strcmp(name, "alpha_narrow_limit")) { if (value < 0 || value > 32767) return 0; dec->alpha_narrow_limit = value; return 1; }
  if (!strcmp(name, "alpha_sample_limit")) { if (value < 0 || value > 255) return 0; dec->alpha_sample_limit = value; return 1; }
  // the alpha path's counters of the last finished batch: groups finished in one pass / groups decoded a second time (-1: not finished)
  if (!strcmp(name, "query_alpha_narrow_groups") || !strcmp(name, "query_alpha_redo_groups")) {
    JxlHipDecoder::Slot& S = dec->Last();
    if (S.pending || !S.h_status) return -1;
    const int word = name[12] == 'n' ? kStatusAlphaNarrow : kStatusAlphaRedo;
    int64_t sum = 0;
    for (int i = 0; i < S.n; i++) sum += S.h_status[(size_t)i * 16 + word];
    return (int32_t)std::min<int64_t>(sum, INT32_MAX);
  }
  // the 64x64 tiles of the last finished batch that recon_tile_kernel left to the generic reconstruction kernels (-1: not finished)
  if (!strcmp(name, "query_generic_tiles")) {
    JxlHipDecoder::Slot& S = dec->Last();
    if (S.pending || !S.h_status) return -1;
    int64_t sum = 0;
    for (int i = 0; i < S.n; i++) sum += S.h_status[(size_t)i * 16 + 1];
    return (int32_t)std::min<int64_t>(sum, INT32_MAX);
  }
  if (!strcmp(name, "no_stream_pairs")) { dec->no_stream_pairs = value != 0; return 1; }
  if (!strcmp(name, "no_lf_pipeline")) { dec->no_lf_pipeline = value != 0; return 1; }
  if (!strcmp(name, "mod_lanes64")) { dec->mod_lanes64 = value != 0; return 1; }
  if (!strcmp(name, "overlap")) { dec->overlap = value != 0; return 1; }
  // 1: full size; 8: the next batches are decoded at 1:8 (2 and 4 are reserved: they need reduced inverse transforms)
  if (!strcmp(name, "downscale")) { if (value != 1 && value != 8) return 0; dec->downscale = value; return 1; }
  return 0;
}

size_t jxlhip_read_plane(JxlHipDecoder* dec, int32_t index, const char* name, int32_t channel, void* dst, size_t capacity) {
  if (!dec || !name) return 0;
  JxlHipDecoder::Slot& S = dec->Last();
  if (index < 0 || index >= S.n || S.pending) return 0;
  if (S.parse_status[index] != DecoderStatus_Ok) return 0;
  const DevImage& d = S.imgs[index];
  std::string nm(name);
  const size_t cells = (size_t)d.w8 * d.h8, pix = (size_t)d.wp * d.hp;
  const void* src = nullptr;
  size_t bytes = 0;
  bool host = false;
  const int c = std::min(2, std::max(0, channel));
  if (nm == "lf") { src = d.lf_final[c]; bytes = cells * 4; }
  else if (nm == "lf_quant") { src = d.lfq[c]; bytes = cells * 4; }
  else if (nm == "cellinfo") { src = d.cellinfo; bytes = cells * 4; }
  else if (nm == "raw_quant") { src = d.rawq; bytes = cells * 2; }
  else if (nm == "sharpness") { src = d.sharp; bytes = cells; }
  else if (nm == "ytox") { src = d.ytox; bytes = (size_t)d.wt * d.ht; }
  else if (nm == "ytob") { src = d.ytob; bytes = (size_t)d.wt * d.ht; }
  else if (nm == "alpha") { src = d.alpha; bytes = (size_t)d.w * d.h; }
  else if (nm == "inv_sigma") { src = d.inv_sigma; bytes = cells * 4; }
  else if (dec->debug_taps && (size_t)index < S.taps.size()) {
    host = true;
    if (nm == "qcoef") { src = S.taps[index].qcoef[c].data(); bytes = S.taps[index].qcoef[c].size(); }
    else if (nm == "xyb_idct") { src = S.taps[index].xyb_idct[c].data(); bytes = S.taps[index].xyb_idct[c].size(); }
    else if (nm == "xyb_filtered") { src = S.taps[index].xyb_filtered[c].data(); bytes = S.taps[index].xyb_filtered[c].size(); }
    else if (nm == "noise_rnd") { src = S.taps[index].noise_rnd[c].data(); bytes = S.taps[index].noise_rnd[c].size(); }
    else if (nm == "noise") { src = S.taps[index].noise[c].data(); bytes = S.taps[index].noise[c].size(); }
  }
  (void)pix;
  if (!src || !bytes) return 0;
  if (dst && capacity) {
    size_t nb = std::min(bytes, capacity);
    if (host) memcpy(dst, src, nb);
    else if (hipMemcpy(dst, src, nb, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  }
  return bytes;
}

int32_t jxlhip_stage_times(JxlHipDecoder* dec, const char** names, float* ms, int32_t capacity) {
  if (!dec) return 0;
  JxlHipDecoder::Slot& S = dec->Last();
  int32_t k = 0;
  for (size_t i = 1; i < S.stage_names.size() && i < S.stage_ms.size() && k < capacity; i++) {
    if (S.stage_ms[i] < 0.f) continue;
    if (names) names[k] = S.stage_names[i].c_str();
    if (ms) ms[k] = S.stage_ms[i];
    k++;
  }
  return k;
}

// Cumulative stage times over all batches finished since the last reset; returns the number of stages, *batches = batch count.
JXLFILETYPEIO_API int32_t jxlhip_stage_totals(JxlHipDecoder* dec, const char** names, float* ms, int32_t capacity, int32_t* batches,
                                              int32_t reset) {
  if (!dec) return 0;
  int32_t k = 0;
  for (size_t i = 0; i < dec->total_names.size() && k < capacity; i++, k++) {
    if (names) names[k] = dec->total_names[i].c_str();
    if (ms) ms[k] = (float)dec->total_ms[i];
  }
  if (batches) *batches = dec->total_batches;
  // the names stay (the caller reads the returned pointers after this call); only the sums restart
  if (reset) { std::fill(dec->total_ms.begin(), dec->total_ms.end(), 0.0); dec->total_batches = 0; }
  return k;
}

// ---------------------------------------------------------------------- LoadImage
static JxlHipDecoder* ThreadDecoder() {
  static thread_local std::unique_ptr<JxlHipDecoder> dec;
  if (!dec) dec.reset(new JxlHipDecoder(-1));
  return dec.get();
}

// Stage times (HIP events) of this thread's last LoadImage: what bench.py reports beside the wall time of the call
extern "C" JXLFILETYPEIO_API int32_t jxlhip_last_load_stage_times(const char** names, float* ms, int32_t capacity) {
  try { return jxlhip_stage_times(ThreadDecoder(), names, ms, capacity); } catch (...) { return 0; }
}

DecoderStatus LoadImage(DecoderCallbacks* cb, const uint8_t* data, size_t size, ErrorInfo* err) {
  if (!cb || !data) return DecoderStatus_NullParameter;   // Decoder/JxlDecoder.cpp:802-805
  DecoderStatus result = DecoderStatus_Ok;
  try {
    // ---- pass 1: basic info, colour profile, metadata boxes (Decoder/JxlDecoder.cpp:412-793)
    ParsedFrame f;
    ParseFile(data, size, true, f);
    if (f.xsize > 0x7FFFFFFFu || f.ysize > 0x7FFFFFFFu) return DecoderStatus_ImageDimensionExceedsInt32;   // :477-481
    int black = 0, alphas = 0;
    for (auto& e : f.ec) { if (e.type == 4) black++; if (e.type == 0) alphas++; }
    if ((f.ncolor != 1 && f.ncolor != 3) || black > 1 || alphas > 1) return DecoderStatus_UnsupportedChannelFormat;   // :485-490
    const bool has_alpha = f.alpha_index >= 0;
    const bool cmyk = black == 1;   // ExtraChannelsAreSupported + DecoderImageFormat::Cmyk (:110-157, :499-503)
    // sample type by bit depth (Decoder/JxlDecoder.cpp:510-556)
    int rep = ImageChannelRepresentation_Uint8;
    if (f.exp_bits > 0) {
      if (f.bits <= 16) rep = ImageChannelRepresentation_Float16;        // :521-525
      else if (f.bits <= 32) rep = ImageChannelRepresentation_Float32;   // :526-530
      else { SetErr(err, "Unsupported floating point bit depth: %u.", f.bits); return DecoderStatus_DecodeError; }   // :531-535
    } else if (f.bits > 8) {
      if (f.bits > 16) { SetErr(err, "Unsupported integer bit depth: %u.", f.bits); return DecoderStatus_DecodeError; }   // :551
      rep = ImageChannelRepresentation_Uint16;
    }
    const bool swap_sides = f.orientation >= 5;   // the host is told the size as displayed
    cb->setBasicInfo((int32_t)(swap_sides ? f.ysize : f.xsize), (int32_t)(swap_sides ? f.xsize : f.ysize),
                     cmyk ? DecoderImageFormat_Cmyk : (f.ncolor == 1 ? DecoderImageFormat_Gray : DecoderImageFormat_Rgb), (ImageChannelRepresentation)rep,
                     has_alpha);   // :558
    // colour encoding -> KnownColorProfile (Decoder/JxlDecoder.cpp:36-108); anything else would take the reference's ICC route
    {
      const ColorPlan plan = PlanColor(f);
      if (plan.report_icc) {   // the target-data profile is the embedded ICC profile (:652-682)
        const std::vector<uint8_t>& prof = f.icc.empty() ? plan.icc_out : f.icc;   // embedded, or synthesised for the enumerated encoding
        if (!prof.empty() && !cb->setIccProfile(const_cast<uint8_t*>(prof.data()), prof.size())) return DecoderStatus_CreateMetadataError;
      } else if (plan.known_profile < 0) {
        SetErr(err, "This colour encoding needs a synthesised ICC profile, which the GPU path does not build yet.");
        return DecoderStatus_DecodeError;
      } else if (!cb->setKnownColorProfile((KnownColorProfile)plan.known_profile)) {
        return DecoderStatus_CreateMetadataError;   // :648-651
      }
    }
    // metadata boxes in file order, whatever their payload size (the reference reports a box when the library completes it, :756-782)
    static uint8_t empty_payload[1] = {0};
    for (auto& b : f.meta_in_order) {
      uint8_t* p = b.size ? const_cast<uint8_t*>(b.data) : empty_payload;
      if (!(b.is_exif ? cb->setExif(p, b.size) : cb->setXmp(p, b.size))) return DecoderStatus_CreateMetadataError;
    }
    // ---- pass 2: the frame (Decoder/JxlDecoder.cpp:217-410)
    JxlHipDecoder* dec = ThreadDecoder();
    const int nch = f.ncolor + (cmyk ? 1 : 0) + (has_alpha ? 1 : 0);   // CMYK: C M Y K [A], inverted for the host on the device (:159-215)
    const size_t bytes = (size_t)f.xsize * f.ysize * nch * OutBytesPerSample(f);   // tightly packed, :291-313
    dec->EnsureLoadImageBuffers(bytes);
    uint8_t* const d_out = dec->li_dev;
    uint8_t* const h_out = dec->li_host;   // valid for the duration of the setLayerData call, like the reference's buffer (:291-313)
    DecoderStatus st = DecoderStatus_Ok;
    const uint8_t* hd = data;
    uint8_t* od = d_out;
    dec->Decode(1, &hd, &size, nullptr, &od, nullptr, true, &st, err);
    if (st != DecoderStatus_Ok) result = st;
    else {
      HIP_OK(hipMemcpy(h_out, d_out, bytes, hipMemcpyDeviceToHost));
      std::vector<char> name;
      if (!f.name.empty()) { name.assign(f.name.begin(), f.name.end()); name.push_back(0); }   // nameLength includes the NUL (:274,369)
      if (!cb->setLayerData(h_out, name.empty() ? nullptr : name.data(), name.size())) result = DecoderStatus_CreateLayerError;   // :384-395
    }
  } catch (const ParseError& e) {
    SetErr(err, "%s", e.what());
    result = e.status;
  } catch (const std::bad_alloc&) {
    result = DecoderStatus_OutOfMemory;
  } catch (const std::exception& e) {
    SetErr(err, "%s", e.what());
    result = DecoderStatus_DecodeError;
  } catch (...) {
    result = DecoderStatus_DecodeError;
  }
  return result;
}

// SaveImage lives in encoder.cc.

}  // extern "C"

// ---------------------------------------------------------------------- animations: every displayed image of a file, in file order
// The state between two displayed images is the four reference slots, so decoding is sequential from an entry point (an image with no
// live slot in front of it; animation.h).  Frames are decoded in chunks: each chunk is one JxlHipDecoder::Decode of a layered file made
// of the chunk's frames, whose compose launch stores the displayed images the chunk's plan selects - at full size, or at 1:8
// (compose_reduce_kernel) - and carries the live slots from and to the slot buffers.
struct JxlHipAnimation {
  std::vector<uint8_t> file;      // the caller's bytes (the parse points into them)
  Animation anim;
  AnimPlan plan;
  ParsedFrame top;                // what every chunk's file looks like from outside: the image header on the canvas
  std::unique_ptr<JxlHipDecoder> dec;
  uint8_t* d_cs = nullptr;        // the codestream, uploaded once
  // The slots that are alive at some cut of the file, one canvas-sized plane of nch floats per pixel each (slot_plane), twice: a chunk
  // loads from d_slots[cur_slots] and stores to the other, and the two swap when the chunk has succeeded - after a failure the state
  // in front of the chunk is intact.  Null when no cut has a live slot.
  float* d_slots[2] = {nullptr, nullptr};
  int slot_plane[4] = {0, 0, 0, 0};
  int cur_slots = 0;
  AnimCursor cur;                 // where the next chunk starts and which image is delivered next (a seek only moves this)
  std::vector<int> entry_points;
  int chunk_frames = 0;
  size_t image_bytes = 0, reduced_bytes = 0;
  int disp_w = 0, disp_h = 0, nch = 0, out_bits = 8, out_float = 0;
  uint8_t* d_single = nullptr;    // a single-frame file's full-size image, for its thumbnail (allocated when first asked for)
  ~JxlHipAnimation() {
    if (dec) (void)hipSetDevice(dec->device);
    if (d_cs) (void)hipFree(d_cs);
    if (d_single) (void)hipFree(d_single);
    for (float* p : d_slots) if (p) (void)hipFree(p);
  }
  // out: where the chunk's first stored image goes (full size, or 1:8 when reduce); a chunk that stores none writes nothing
  DecoderStatus RunChunk(const AnimChunk& c, uint8_t* out, bool reduce, ErrorInfo* err);
  DecoderStatus Deliver(int n, int step, bool reduce, uint8_t* out, int32_t* written, ErrorInfo* err);
};

DecoderStatus JxlHipAnimation::RunChunk(const AnimChunk& c, uint8_t* out, bool reduce, ErrorInfo* err) {
  if (anim.single) {   // one single-frame image: the ordinary decode, straight into the caller's buffer
    if (c.stored == 0) return DecoderStatus_Ok;
    // its thumbnail: the same decode into scratch, then the cell means of what it stored (reduce_displayed_kernel)
    if (reduce && !d_single) HIP_OK(hipMalloc(&d_single, std::max<size_t>(image_bytes, 16)));
    uint8_t* full = reduce ? d_single : out;
    ParsedFrame one = anim.frames[0];
    const uint8_t* host = nullptr;
    const size_t size = 0;
    const uint8_t* dev = d_cs;
    DecoderStatus st = DecoderStatus_Ok;
    ErrorInfo detail;
    detail.errorMessage[0] = 0;
    dec->Decode(1, &host, &size, &dev, &full, nullptr, true, &st, &detail, &one);
    if (st != DecoderStatus_Ok) SetErr(err, "animation, codestream frame 0: %s", detail.errorMessage);
    if (st == DecoderStatus_Ok && reduce) {
      // (Decode has waited for its stream; the call returns when the means are stored)
      LaunchReduceDisplayed(d_single, out, disp_w, disp_h, nch, out_bits, out_float, nullptr);
      HIP_OK(hipGetLastError());
      HIP_OK(hipStreamSynchronize(nullptr));
    }
    return st;
  }
  ParsedFrame file = top;
  auto lay = std::make_shared<Layers>();
  lay->canvas_w = top.xsize; lay->canvas_h = top.ysize;
  lay->raw = anim.raw;
  lay->frames.assign(anim.frames.begin() + c.first, anim.frames.begin() + c.first + c.count);
  lay->save.assign(anim.save.begin() + c.first, anim.save.begin() + c.first + c.count);
  for (int k = 0; k < c.count; k++) {   // the images the plan selects, in the order they lie in `out`; every other frame stores nothing
    const int j = anim.show[c.first + k];
    const bool stored = j >= 0 && c.first_stored >= 0 && j >= c.first_stored && (j - c.first_stored) % c.step == 0;
    lay->show.push_back(stored ? (j - c.first_stored) / c.step : -1);
  }
  lay->reduce = reduce;
  lay->live_in = c.live_in; lay->live_out = c.live_out;
  lay->slots_in = d_slots[cur_slots]; lay->slots_out = d_slots[cur_slots ^ 1];
  for (int s = 0; s < 4; s++) lay->slot_plane[s] = slot_plane[s];
  lay->out_stride = reduce ? reduced_bytes : image_bytes;
  file.layers = lay;
  const uint8_t* host = nullptr;
  const size_t size = 0;
  const uint8_t* dev = d_cs;
  DecoderStatus st = DecoderStatus_Ok;
  ErrorInfo detail;
  detail.errorMessage[0] = 0;
  dec->Decode(1, &host, &size, &dev, &out, nullptr, true, &st, &detail, &file);
  if (st == DecoderStatus_Ok) cur_slots ^= 1;   // what the chunk stored is the state now
  if (st != DecoderStatus_Ok) {
    // the chunk's images are its frames: the first one that failed names the codestream frame
    JxlHipDecoder::Slot& S = dec->Last();
    int bad = 0;
    for (int i = 0; i < S.n; i++)
      if (S.parse_status[i] != DecoderStatus_Ok || S.h_status[(size_t)i * 16]) { bad = i; break; }
    SetErr(err, "animation, codestream frame %d: %s", c.first + bad, detail.errorMessage);
  }
  return st;
}

// n images, every step-th from the position on, into `out` (image_bytes or reduced_bytes apart): DeliverImages' chunks, each one Decode.
DecoderStatus JxlHipAnimation::Deliver(int n, int step, bool reduce, uint8_t* out, int32_t* written, ErrorInfo* err) {
  DecoderStatus st = DecoderStatus_Ok;
  try {
    const size_t stride = reduce ? reduced_bytes : image_bytes;
    DeliverImages(anim, plan, cur, n, step, chunk_frames, kAnimChunkScratch, [&](const AnimChunk& c, int done) {
      st = RunChunk(c, out + (size_t)done * stride, reduce, err);
      if (st == DecoderStatus_Ok && written) *written = done + c.stored;
      return st == DecoderStatus_Ok;   // after a failure the position stays in front of the chunk
    });
    return st;
  } catch (const std::bad_alloc&) {
    return DecoderStatus_OutOfMemory;
  } catch (const std::exception& e) {
    SetErr(err, "%s", e.what());
    return DecoderStatus_DecodeError;
  }
}

extern "C" {

JxlHipAnimation* jxlhip_animation_open(int32_t device, const uint8_t* data, size_t size, JxlHipAnimationInfo* info, ErrorInfo* err) {
  if (!data) { SetErr(err, "null file"); return nullptr; }
  try {
    // everything the parser refuses is refused here, before any HIP call
    std::unique_ptr<JxlHipAnimation> a(new JxlHipAnimation());
    a->file.assign(data, data + size);
    ParseAnimation(a->file.data(), a->file.size(), false, a->anim);
    a->plan = PlanAnimation(a->anim);
    a->entry_points = EntryPoints(a->anim, a->plan);
    ParsedFrame& head = a->anim.head;
    {
      auto cs_copy = std::move(head.cs_copy);
      auto owned = std::move(head.owned_boxes);
      a->top = head;
      head.cs_copy = std::move(cs_copy);
      head.owned_boxes = std::move(owned);
    }
    for (auto& fr : a->anim.frames) { fr.cs_file_offset = 0; fr.cs_contiguous = true; }   // d_cs holds the codestream itself
    const size_t nch = OutSamplesPerPixel(head);
    a->image_bytes = (size_t)head.xsize * head.ysize * nch * OutBytesPerSample(head);
    a->disp_w = (int)(head.orientation >= 5 ? head.ysize : head.xsize); a->disp_h = (int)(head.orientation >= 5 ? head.xsize : head.ysize);
    a->nch = (int)nch; a->out_bits = 8 * (int)OutBytesPerSample(head); a->out_float = head.exp_bits ? 1 : 0;
    a->reduced_bytes = (size_t)((a->disp_w + 7) / 8) * ((a->disp_h + 7) / 8) * nch * OutBytesPerSample(head);
    int live = 0, nslots = 0;
    for (int m : a->plan.live_after) live |= m;
    for (int s = 0; s < 4; s++) if (live >> s & 1) a->slot_plane[s] = nslots++;
    a->dec.reset(new JxlHipDecoder(device));
    a->dec->single_slot = true;
    HIP_OK(hipMalloc(&a->d_cs, head.cs_size + 16));
    HIP_OK(hipMemcpy(a->d_cs, head.cs, head.cs_size, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(a->d_cs + head.cs_size, 0, 16));
    for (float*& p : a->d_slots) if (nslots) HIP_OK(hipMalloc(&p, (size_t)nslots * head.xsize * head.ysize * nch * sizeof(float)));
    if (info) {
      memset(info, 0, sizeof(*info));
      info->width = head.orientation >= 5 ? head.ysize : head.xsize; info->height = head.orientation >= 5 ? head.xsize : head.ysize;
      info->has_alpha = head.alpha_index >= 0;
      info->num_channels = (int32_t)nch;
      info->bytes_per_sample = (int32_t)OutBytesPerSample(head);
      info->float_samples = head.exp_bits ? 1 : 0;
      info->bits_per_sample = (int32_t)head.bits;
      info->have_animation = head.have_animation;
      info->tps_numerator = head.tps_numerator; info->tps_denominator = head.tps_denominator; info->num_loops = head.num_loops;
      info->have_timecodes = head.have_timecodes;
      info->num_displayed = (int32_t)a->anim.completes.size();
      info->num_codestream_frames = (int32_t)a->anim.frames.size();
      info->image_bytes = a->image_bytes;
    }
    return a.release();
  } catch (const std::exception& e) {
    SetErr(err, "%s", e.what());
    return nullptr;
  }
}

void jxlhip_animation_close(JxlHipAnimation* a) { delete a; }

JxlHipDecoder* jxlhip_animation_decoder(JxlHipAnimation* a) { return a ? a->dec.get() : nullptr; }

int32_t jxlhip_animation_frame(JxlHipAnimation* a, int32_t j, JxlHipAnimationFrame* out) {
  if (!a || !out || j < 0 || j >= (int32_t)a->anim.completes.size()) return 0;
  const int k = a->anim.completes[j];
  const ParsedFrame& fr = a->anim.frames[k];
  memset(out, 0, sizeof(*out));
  out->duration = fr.duration; out->timecode = fr.timecode;
  out->first_codestream_frame = j > 0 ? a->anim.completes[j - 1] + 1 : 0;
  out->num_codestream_frames = k + 1 - out->first_codestream_frame;
  out->name_length = (int32_t)std::min(fr.name.size(), sizeof(out->name) - 1);
  memcpy(out->name, fr.name.data(), (size_t)out->name_length);
  return 1;
}

DecoderStatus jxlhip_animation_next(JxlHipAnimation* a, int32_t count, void* dev_out, size_t capacity, int32_t* written, ErrorInfo* err) {
  if (written) *written = 0;
  if (!a || (count > 0 && !dev_out)) return DecoderStatus_NullParameter;
  const int n = SelectedImages(a->anim, a->cur, count, 1);
  if ((size_t)n > capacity / std::max<size_t>(1, a->image_bytes)) {
    SetErr(err, "the buffer holds %zu bytes, %d displayed images need %zu", capacity, n, (size_t)n * a->image_bytes);
    return DecoderStatus_InvalidParameter;
  }
  return a->Deliver(n, 1, false, (uint8_t*)dev_out, written, err);
}

DecoderStatus jxlhip_animation_next_reduced(JxlHipAnimation* a, int32_t count, int32_t step, void* dev_out, size_t capacity, int32_t* written,
                                            ErrorInfo* err) {
  if (written) *written = 0;
  if (!a || (count > 0 && !dev_out)) return DecoderStatus_NullParameter;
  if (step < 1) {
    SetErr(err, "step %d: every step-th image from the position on, step >= 1", step);
    return DecoderStatus_InvalidParameter;
  }
  const int n = SelectedImages(a->anim, a->cur, count, step);
  if ((size_t)n > capacity / std::max<size_t>(1, a->reduced_bytes)) {
    SetErr(err, "the buffer holds %zu bytes, %d displayed images at 1:8 need %zu", capacity, n, (size_t)n * a->reduced_bytes);
    return DecoderStatus_InvalidParameter;
  }
  return a->Deliver(n, step, true, (uint8_t*)dev_out, written, err);
}

DecoderStatus jxlhip_animation_seek(JxlHipAnimation* a, int32_t j, ErrorInfo* err) {
  if (!a) return DecoderStatus_NullParameter;
  if (!SeekCursor(a->anim, a->entry_points, a->cur, j)) {
    SetErr(err, "seek to displayed image %d: the file has %d (0 .. %d, %d: the end)", j, (int)a->anim.completes.size(), (int)a->anim.completes.size() - 1,
           (int)a->anim.completes.size());
    return DecoderStatus_InvalidParameter;
  }
  return DecoderStatus_Ok;
}

int32_t jxlhip_animation_entry_points(JxlHipAnimation* a, int32_t* displayed, int32_t capacity) {
  if (!a) return 0;
  if (displayed)
    for (int32_t i = 0; i < capacity && i < (int32_t)a->entry_points.size(); i++) displayed[i] = a->entry_points[i];
  return (int32_t)a->entry_points.size();
}

void jxlhip_animation_position(JxlHipAnimation* a, int32_t* next_codestream_frame, int32_t* next_displayed) {
  if (next_codestream_frame) *next_codestream_frame = a ? a->cur.frame : 0;
  if (next_displayed) *next_displayed = a ? a->cur.shown : 0;
}

void jxlhip_animation_rewind(JxlHipAnimation* a) {
  if (a) (void)SeekCursor(a->anim, a->entry_points, a->cur, 0);   // (image 0's chunk loads no slot: nothing of the old state is read)
}

int32_t jxlhip_animation_set_option(JxlHipAnimation* a, const char* name, int32_t value) {
  if (!a || !name) return 0;
  if (!strcmp(name, "chunk_frames")) { if (value < 0) return 0; a->chunk_frames = value; return 1; }
  // of the decoder's options, those that choose between launch shapes with the same output; neither a band nor a reduced size is
  // offered here, and nothing that changes the layout the chunk plan measured (debug_taps)
  for (const char* ok : {"lane_stride", "no_direct", "mod_lanes64", "no_stream_pairs", "no_lf_pipeline"})
    if (!strcmp(name, ok)) return jxlhip_set_option(a->dec.get(), name, value);
  return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------- host-only introspection (CPU tests)
extern "C" {

// Metadata boxes as LoadImage would hand them to the host (no GPU): which = 0 Exif, k >= 1 the k-th `xml ` box.  Returns the payload
// size (0: absent) and copies up to `capacity` bytes.
JXLFILETYPEIO_API size_t jxlhip_parse_metadata(const uint8_t* data, size_t size, int32_t which, uint8_t* dst, size_t capacity, DecoderStatus* status,
                                               ErrorInfo* err) {
  if (status) *status = DecoderStatus_Ok;
  if (!data) { if (status) *status = DecoderStatus_NullParameter; return 0; }
  try {
    ParsedFrame f;
    ParseFile(data, size, true, f);
    const uint8_t* p = nullptr;
    size_t n = 0;
    if (which == 0) { p = f.exif; n = f.exif_size; }
    else if (which >= 1 && (size_t)which <= f.xml.size()) { p = f.xml[which - 1].first; n = f.xml[which - 1].second; }
    if (p && dst && capacity) memcpy(dst, p, std::min(n, capacity));
    return p ? n : 0;
  } catch (const ParseError& e) {
    SetErr(err, "%s", e.what());
    if (status) *status = (DecoderStatus)e.status;
  } catch (const std::exception& e) {
    SetErr(err, "%s", e.what());
    if (status) *status = DecoderStatus_DecodeError;
  }
  return 0;
}

// Full host-side parse (no GPU): returns the status and a few facts about the parsed tables.
// facts[0..7] = tree nodes, modular clusters, modular log_alpha, AC clusters, AC log_alpha, AC contexts, presets, sections
JXLFILETYPEIO_API DecoderStatus jxlhip_parse_check(const uint8_t* data, size_t size, int32_t* facts, ErrorInfo* err) {
  if (!data) return DecoderStatus_NullParameter;
  try {
    ParsedFrame f;
    ParseFile(data, size, false, f);
    if (facts) {
      facts[0] = (int32_t)f.tree.size(); facts[1] = f.mcode.num_hist; facts[2] = f.mcode.log_alpha;
      facts[3] = f.acode.num_hist; facts[4] = f.acode.log_alpha; facts[5] = (int32_t)f.acode.ctx_map.size();
      facts[6] = f.num_presets; facts[7] = (int32_t)f.sec_off.size();
    }
    return DecoderStatus_Ok;
  } catch (const ParseError& e) {
    SetErr(err, "%s", e.what());
    return e.status;
  } catch (const std::exception& e) {
    SetErr(err, "%s", e.what());
    return DecoderStatus_DecodeError;
  }
}

// Host-only: the embedded ICC profile as LoadImage would hand it to setIccProfile (0: the stream has none).
JXLFILETYPEIO_API size_t jxlhip_parse_icc(const uint8_t* data, size_t size, uint8_t* dst, size_t capacity, DecoderStatus* status, ErrorInfo* err) {
  if (status) *status = DecoderStatus_Ok;
  if (!data) { if (status) *status = DecoderStatus_NullParameter; return 0; }
  try {
    ParsedFrame f;
    ParseFile(data, size, true, f);
    if (dst && capacity) memcpy(dst, f.icc.data(), std::min(f.icc.size(), capacity));
    return f.icc.size();
  } catch (const ParseError& e) {
    SetErr(err, "%s", e.what());
    if (status) *status = (DecoderStatus)e.status;
  } catch (const std::exception& e) {
    SetErr(err, "%s", e.what());
    if (status) *status = DecoderStatus_DecodeError;
  }
  return 0;
}

// Host-only test hooks of icc.cc: the predicted stream -> profile (returns the size, 0 on failure), and the colour model of a
// matrix / TRC profile (model[0..8] linear sRGB -> profile RGB, model[9..17] the inverse; returns 1 if the profile is of that kind).
JXLFILETYPEIO_API size_t jxlhip_icc_unpredict(const uint8_t* enc, size_t size, uint8_t* dst, size_t capacity, ErrorInfo* err) {
  std::vector<uint8_t> e(enc, enc + size), out;
  std::string why;
  if (!IccUnpredict(e, &out, &why)) { SetErr(err, "%s", why.c_str()); return 0; }
  if (dst && capacity) memcpy(dst, out.data(), std::min(out.size(), capacity));
  return out.size();
}
JXLFILETYPEIO_API int32_t jxlhip_icc_model(const uint8_t* icc, size_t size, double* model, float* to_linear, float* from_linear) {
  IccModel m;
  if (!IccBuildModel(icc, size, &m)) return 0;
  for (int k = 0; k < 9; k++) { model[k] = m.from_linear_srgb[k]; model[9 + k] = m.to_linear_srgb[k]; }
  if (to_linear) for (int c = 0; c < 3; c++) memcpy(to_linear + 256 * c, m.to_linear[c].data(), 256 * 4);
  if (from_linear) for (int c = 0; c < 3; c++) memcpy(from_linear + kIccInvLut * c, m.from_linear[c].data(), kIccInvLut * 4);
  return m.gray ? 2 : 1;
}

// Host-only: byte sizes of the TOC sections in logical order (LfGlobal, LF groups, HfGlobal, pass groups).  Returns their number.
JXLFILETYPEIO_API int32_t jxlhip_section_sizes(const uint8_t* data, size_t size, uint32_t* dst, int32_t capacity) {
  if (!data) return 0;
  try {
    ParsedFrame f;
    ParseFile(data, size, true, f);
    const int32_t n = (int32_t)f.sec_size.size();
    for (int32_t i = 0; i < n && i < capacity && dst; i++) dst[i] = f.sec_size[i];
    return n;
  } catch (...) {
    return 0;
  }
}

// name: "natural_order" (index = order bucket, uint16), "dequant" (index = quant table, float, 3*n),
//       "basis" (index = log2(N/8), float N*N).  Returns the byte size.
JXLFILETYPEIO_API size_t jxlhip_static_table(const char* name, int32_t index, void* dst, size_t capacity) {
  const StaticTables& st = GetStaticTables();
  const void* src = nullptr;
  size_t bytes = 0;
  std::string nm(name ? name : "");
  if (nm == "natural_order" && index >= 0 && index < kNumOrders) { src = st.natural_order[index].data(); bytes = st.natural_order[index].size() * 2; }
  else if (nm == "dequant" && index >= 0 && index < kNumQuantTables) { src = st.dq[index].data(); bytes = st.dq[index].size() * 4; }
  else if (nm == "basis" && index >= 0 && index < 6) { src = st.basis[index].data(); bytes = st.basis[index].size() * 4; }
  if (src && dst) memcpy(dst, src, std::min(bytes, capacity));
  return bytes;
}

}  // extern "C"
