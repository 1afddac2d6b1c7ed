// The memory of one decode batch, stated once: which tables go into the uploaded blob, which planes into the workspace, how large each
// is, what type it holds and which DevImage field points at it.  BuildBatch runs twice over the same code: once measuring (regions
// without a base: sizes add up, nothing is written) and once placing (regions with their bases, exactly as large as measured).  Pure
// arithmetic on base addresses: no HIP calls, so the CPU suite checks it (tests/test_batch_layout.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>
#include "entropy_plan.h"

namespace jxlhip {

static inline size_t Align(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Memory handed out front to back.  Measuring (default-constructed): addresses count from 0 and are never dereferenced.  Placing: `host`
// is where bytes are written (null: a region the host never writes, like the workspace), `dev` what the device will see there; an
// allocation that would end past `cap` throws before anything is written.  A measuring region's first allocation has address 0: code that
// lays out must not take a null pointer of a region for "absent" - it keeps that in a flag (as BuildBatch does), or the passes disagree.
struct Region {
  struct Entry { int region; size_t off, bytes, align; };
  int id = 0;
  uint8_t* host = nullptr;
  uintptr_t dev = 0;
  size_t off = 0, cap = 0;
  bool placing = false;
  std::vector<Entry>* log = nullptr;   // tests: every allocation, in order

  Region() = default;
  Region(uint8_t* host_base, const void* dev_base, size_t capacity) : host(host_base), dev((uintptr_t)dev_base), cap(capacity), placing(true) {}

  size_t Take(size_t bytes, size_t align = 256) {
    const size_t at = Align(off, align);
    if (placing && (at > cap || bytes > cap - at)) throw std::length_error("batch layout: an allocation ends past the measured size of its region");
    if (log) log->push_back(Entry{id, at, bytes, align});
    off = at + bytes;
    return at;
  }
  // count elements nobody fills here; the device address
  template <class T> T* Array(size_t count, size_t align = 256) { return reinterpret_cast<T*>(dev + Take(sizeof(T) * count, align)); }
  // count elements that fill(host address) writes; it runs only when there is somewhere to write
  template <class T, class F> const T* Fill(size_t count, F&& fill, size_t align = 256) {
    const size_t at = Take(sizeof(T) * count, align);
    if (host) fill(reinterpret_cast<T*>(host + at));
    return reinterpret_cast<const T*>(dev + at);
  }
  // a copy of src[0 .. count), in an allocation of at least `reserve` elements
  template <class T> const T* Put(const T* src, size_t count, size_t reserve = 0) {
    return Fill<T>(std::max(count, reserve), [&](T* h) { if (count) memcpy(h, src, sizeof(T) * count); });
  }
  // offset of device address p from the region's base
  size_t OffsetOf(const void* p) const { return (size_t)((uintptr_t)p - dev); }
  // where the host writes what the device reads at p (null when measuring)
  template <class T> T* Host(const T* p) const { return host ? reinterpret_cast<T*>(host + ((uintptr_t)p - dev)) : nullptr; }
};

// Element i of an array a region handed out (measuring: its base may be 0, so the address is formed as an integer)
template <class T> static inline T* ElementAt(T* base, size_t i) { return reinterpret_cast<T*>((uintptr_t)base + i * sizeof(T)); }

struct BatchRegions {
  Region blob;   // tables, descriptors, uploaded codestreams: filled on the host, copied to the device in one piece
  Region zero;   // the head of the workspace that is cleared for every batch (status words, cell info)
  Region ws;     // behind it: the planes and scratch of each image
  Region pix;    // behind those: the planes that chunks of frames share in the pixel stages
  size_t ZeroBytes() const { return Align(zero.off, 256); }
  size_t PixStart() const { return ZeroBytes() + Align(ws.off, 256); }   // from the start of the workspace
  size_t WorkspaceBytes() const { return PixStart() + pix.off; }
};

// A layered file of the batch: its frames are images [first, first + count) of the batch, compose_kernel blends them into `out`.
struct Composite { int file, first, count; std::vector<int> save; uint8_t* out; };

// The patch dictionaries of the batch's patched frames, positions listed per 64x64 tile in dictionary order (patch_kernel).  The
// device pointers (PatchFrame::px, PatchRef::px) are filled in by BuildBatch.
struct PatchTables {
  std::vector<int> image, first;   // per PatchFrame: its image of the batch, and image 0 of its file (PatchRect::frame counts from there)
  std::vector<PatchRef> refs;
  std::vector<PatchPos> pos;
  std::vector<PatchTile> tiles;
  std::vector<int32_t> list;
};
PatchTables BuildPatchTables(const std::vector<ParsedFrame>& frames, const std::vector<int>& parse_status, const std::vector<Composite>& comps);

struct BatchInput {
  const std::vector<ParsedFrame>* frames = nullptr;
  const std::vector<int>* parse_status = nullptr;
  const EntropyPlan* plan = nullptr;
  const uint8_t* const* dev_data = nullptr;   // null, or per image: the file in device memory (null: upload the codestream)
  uint8_t* const* dev_out = nullptr;
  // layered files: their composites and patches, the file of each image (empty: one image per file), the parse of each layered file
  const std::vector<Composite>* comps = nullptr;
  const PatchTables* patches = nullptr;
  const std::vector<int>* file_of = nullptr;
  const std::vector<ParsedFrame>* files = nullptr;
  int nfiles = 0;
  // the decoder's static tables (device)
  const uint16_t* const* d_natural = nullptr;
  const U32x2* const* d_scan = nullptr;
  const float* const* d_dq = nullptr;
  const uint32_t* dq_n = nullptr;
  bool ds = false, debug_taps = false, no_stream_pairs = false;
  int pixel_chunk_cap = 32;
};

// One inverse transform of a Modular frame that is a launch of its own (Squeeze, palette, RCTs beside them).
struct ModLaunch { int kind; int32_t *a, *b, *c; int aw, ah, rw, rh, type; int32_t* out[4]; int nout; uint32_t* status; };

// Everything the enqueue section reads.
struct BatchOutput {
  std::vector<DevImage> imgs;       // host copies (device pointers inside): the batch's images, then the later passes' records
  std::vector<size_t> status_off;   // offset of each image's status words in the workspace (the zeroed head starts it)
  std::vector<ModLaunch> mod_ops;
  bool any_alpha = false, any_unfiltered = false, any_noise = false, any_vardct = false;
  int stage_mask = 0;   // LDS-tiled loop-filter stage kernels some frame of the batch needs (bit s: filter_tile_kernel<s>)
  int any_fused = 0, any_fused2 = 0;   // 1: fused frames (with a second iteration) of the two-pixels-per-lane kernels, 2: others
  int max_w = 1, max_h = 1, max_tiles = 1, max_groups = 1, max_segments = 1;
  bool compose_reduce = false;   // the batch's layered images leave at 1:8 (an animation's thumbnails: a batch of one)
  int max_reduce_cells = 1;
  size_t max_cells = 1, max_ds_cells = 1, max_mod_pixels = 1;   // max_ds_cells: reduced-size decode, over the frames of both kinds
  int pixel_chunk = 1;   // frames that share one set of reconstruction / filter planes are this far apart
  DevImage* d_imgs = nullptr;           // where imgs goes in the blob
  uint32_t* status_base = nullptr;      // 16 words per image, side by side
  const SectionTask *lf_tasks = nullptr, *pass_tasks = nullptr, *lf_ans_tasks = nullptr, *mod_tasks = nullptr, *alpha_tasks = nullptr;
  const ComposeImage* comp_imgs = nullptr;
  const ComposeFrame* comp_frames = nullptr;
  const PatchFrame* patch_frames = nullptr;
  const PatchRef* patch_refs = nullptr;
  const PatchPos* patch_pos = nullptr;
  const PatchTile* patch_tiles = nullptr;
  const int32_t* patch_list = nullptr;
};

// Bytes per output sample: the sample type follows the colour channels' depth (Decoder/JxlDecoder.cpp:510-556): u8, u16, f16, f32.
static inline size_t OutBytesPerSample(const ParsedFrame& f) { return f.exp_bits ? (f.bits <= 16 ? 2 : 4) : (f.bits > 8 ? 2 : 1); }
// Interleaved output samples per pixel: colour, black, alpha.  (Only a lone Modular frame can have a black channel: the parser refuses
// layered CMYK files, so for a frame of a layered or patched file this is colour + alpha.)
static inline size_t OutSamplesPerPixel(const ParsedFrame& f) { return (size_t)f.ncolor + (f.black_index >= 0 ? 1 : 0) + (f.alpha_index >= 0 ? 1 : 0); }

// Scan list of quant table q: for each channel (X, Y, B) and scan position k, the stored-layout index order[k] and the bits of the
// dequantisation weight at that index; 3 * (entries of the table) records go to out.  custom: the frame's own coefficient orders
// ([bucket][channel], empty = natural), custom_dq: its own weights (null: the library table).
void BuildScanList(int q, const std::vector<uint16_t> (*custom)[3], U32x2* out, const std::vector<float>* custom_dq = nullptr);

// The tables of an entropy code go into the blob; dc describes them: context map, packed cfg words (with the single-symbol forms),
// alias tables, a prefix code's counts / symbol offsets / sorted symbols, the LZ77 fields.
void PackCode(const HostCode& hc, Region& blob, DevCode& dc);

// Lays out one batch.  `out` must be fresh; R's regions must all be measuring or all be placing.
void BuildBatch(const BatchInput& in, BatchRegions& R, BatchOutput& out);

}  // namespace jxlhip
