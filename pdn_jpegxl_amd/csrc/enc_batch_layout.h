// The device buffers of one image being encoded, stated once, and the workspace of a batch of them (jxlhip_encode_batch).
//
// The Lay* templates list every buffer an EncImage needs and its size; they ask an allocator for them.  SaveImage / jxlhip_save_pixels
// run them over the Arena of the call (one hipMalloc each, encoder.cc); LayEncBatch runs the same lists over a carver of the batch
// encoder's single workspace, once without a base to measure and once with the base to place - there is no second size formula.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "enc_types.h"

namespace jxlhip {

// Counters and histograms are asked for by kind, so that a batch can keep each kind of all its images together: the histograms come
// down in one copy, so do the section sizes, and the whole head is cleared by one memset.
enum EncCounterKind { kEncHist = 0, kEncSecBits = 1, kEncCount = 2, kNumEncCounterKinds = 3 };

void SetEncGeometry(uint32_t w, uint32_t h, EncImage& im);

inline int EncNumSections(const EncImage& im) { return im.lossless ? im.ng : im.nlf + im.ng + 1; }   // lossy: + the global alpha stream
inline size_t EncNumStreamStates(const EncImage& im) { return (size_t)2 * (im.nlf + im.ng) + 1; }

// lossy: planes of the front end (geometry, gray and has_alpha are set)
template <class Alloc>
void LayLossyPlanes(Alloc& a, EncImage& im) {
  const size_t npx = (size_t)im.w * im.h, npad = (size_t)im.wp * im.hp, ncell = (size_t)im.w8 * im.h8;
  for (int c = 0; c < 3; c++) {
    im.xyb[c] = a.template Get<float>(npx);
    im.pad[c] = a.template Get<float>(npad);
    im.lfq[c] = a.template Get<int32_t>(ncell);
    im.qs[c] = a.template Get<int32_t>(ncell * 64);
    im.nz[c] = a.template Get<uint8_t>(ncell);
    im.nzc[c] = a.template Get<uint16_t>(ncell);
    im.last[c] = a.template Get<uint16_t>(ncell);
  }
  im.rawq = a.template Get<int32_t>(ncell);
  im.act = a.template Get<float>(ncell);
  im.strat = a.template Get<uint8_t>(ncell);
  if (im.has_alpha) im.alpha_px = a.template Get<int32_t>(npx);
  if (im.cfl) {   // fitted chroma-from-luma maps: one value per 64x64 tile (an image without them lays out what it always did)
    const size_t ntile = (size_t)((im.w8 + 7) / 8) * ((im.h8 + 7) / 8);
    im.ytox = a.template Get<int8_t>(ntile);
    im.ytob = a.template Get<int8_t>(ntile);
  }
}

// lossy: everything that follows from the quantised data - tokens, counters, histograms, section buffers
template <class Alloc>
void LayLossyCoding(Alloc& a, EncImage& im) {
  im.meta_cap = kMetaTokCap + (im.cfl ? kCflTokCap : 0);
  im.tok_lf = a.template Get<DevToken>((size_t)im.nlf * kLfTokCap);
  im.tok_meta = a.template Get<DevToken>((size_t)im.nlf * im.meta_cap);
  im.tok_ac = a.template Get<DevToken>((size_t)im.ng * kAcTokCap);
  if (im.has_alpha) im.tok_alpha = a.template Get<DevToken>((size_t)im.ng * kAlphaTokCap);
  im.n_ac = a.template Counter<uint32_t>(kEncCount, im.ng);
  im.n_meta = a.template Counter<uint32_t>(kEncCount, im.nlf);
  im.hist_mod = a.template Counter<uint32_t>(kEncHist, kNumEncLeaves * kEncSyms);
  im.hist_ac = a.template Counter<uint32_t>(kEncHist, (size_t)kAcContexts * kEncSyms);
  const int nsec = EncNumSections(im);
  im.sec_cap = ((size_t)std::max(kLfTokCap + im.meta_cap, kAcTokCap + kAlphaTokCap) * kSecBytesPerTok + 256) & ~(size_t)15;
  im.sec_bytes = a.template Get<uint8_t>((size_t)nsec * im.sec_cap);
  im.sec_bits = a.template Counter<uint64_t>(kEncSecBits, nsec);
  im.stream_state = a.template Counter<uint32_t>(kEncCount, EncNumStreamStates(im));
}

// lossless: channel planes and tokens (ll_nch is set)
template <class Alloc>
void LayLosslessPlanes(Alloc& a, EncImage& im) {
  const size_t npx = (size_t)im.w * im.h;
  for (int c = 0; c < im.ll_nch; c++) im.ll_plane[c] = a.template Get<int32_t>(npx);
  im.tok_ll = a.template Get<DevToken>((size_t)im.ng * kLlTokCap);
}
// lossless, fixed stream: the section buffers (one per group) and their counters
template <class Alloc>
void LayLosslessSections(Alloc& a, EncImage& im) {
  const int nsec = EncNumSections(im);
  im.sec_cap = ((size_t)kLlTokCap * kSecBytesPerTok + 256) & ~(size_t)15;
  im.sec_bytes = a.template Get<uint8_t>((size_t)nsec * im.sec_cap);
  im.sec_bits = a.template Counter<uint64_t>(kEncSecBits, nsec);
  im.stream_state = a.template Counter<uint32_t>(kEncCount, EncNumStreamStates(im));
}

// Most bytes an entropy code takes in device memory, packed as PackEncCode (encoder.cc) packs it: per cluster the frequencies, the
// cumulative starts and the 4096-entry slot map, 16 bits each; one byte per context; four 256-byte alignments.
constexpr size_t EncCodeBytes(size_t clusters, size_t contexts) { return clusters * (2 * kEncSyms * 2 + 4096 * 2) + contexts + 4 * 256; }
constexpr int kEncModClusters = 8, kEncHfClusters = 64;   // cluster caps of the lossy codes (the lossless fixed code: 4)
constexpr size_t kEncModCodeBytes = EncCodeBytes(kEncModClusters, kNumEncLeaves);
constexpr size_t kEncHfCodeBytes = EncCodeBytes(kEncHfClusters, kAcContexts);

// ---- the batch
struct EncBatchItem {
  uint32_t w, h;
  int32_t nch;            // 1..4 interleaved samples per pixel
  int32_t sample_bytes;   // 1, 2 or 4
  int32_t lossless;
  int32_t cfl;            // lossy: chroma-from-luma maps fitted per tile (JxlHipLossyOptions::chroma_from_luma)
};
// where the buffers of one image lie that are no field of its EncImage (offsets from the workspace base)
struct EncBatchSlot {
  size_t src;        // the caller's pixels in tight rows: w * nch * sample_bytes * h
  size_t surface;    // the BGRA8 surface of 8-bit input: w * 4 * h (deeper input: unused, = src)
  size_t begin, end; // the image's own part of the body (its head entries apart)
};
// Behind the head come the small pieces the host uploads, ordered so that each upload is one copy: the kernels' tables, the records
// as the kernels of the Modular streams read them and the Modular codes (known together, first); the records as the later kernels read
// them and the HF codes (known together, second); the compaction's offsets (known last).  The records are two arrays because the
// first is being read by running kernels when the second goes up.
struct EncBatchLayout {
  size_t region[kNumEncCounterKinds + 1];   // first byte of the histograms, the section sizes, the counters, and the end of the head
  size_t head_bytes;     // = region[kNumEncCounterKinds]: cleared per batch by one memset
  size_t tables;         // (first, image_of, wg0) of the batch kernels: kEncBatchTables * 3 arrays of up to 2 n entries each
  size_t records_m;      // n EncImage records, mcode set
  size_t mcodes;         // the Modular codes, packed: room for the worst case of every image
  size_t records_a;      // n EncImage records, mcode and acode set
  size_t acodes;         // the HF codes of the lossy images, packed: room for the worst case
  size_t dst_off;        // one uint64 per section of the batch: where the compaction puts it
  size_t body;           // the images' buffers
  size_t total_sections; // of all images
  size_t total_bytes;
  std::vector<EncBatchSlot> slots;
};
constexpr int kEncBatchTables = 6;   // reverse (Modular streams), reverse (HF streams), section layout, lossless sections, global alpha, compaction
inline size_t EncBatchTableStride(int n) { return (((size_t)n * 2 * 4) + 255) & ~(size_t)255; }   // bytes from one array of a table to the next

// Lays out the workspace of a batch.  base == nullptr: measure (the pointers written into `ims` are offsets); otherwise place.  Both
// run the same code, so they agree.  ims[i] gets its geometry, gray, has_alpha, lossless, ll_nch and every buffer pointer.
void LayEncBatch(const EncBatchItem* items, int n, uint8_t* base, EncImage* ims, EncBatchLayout* lay);

}  // namespace jxlhip
