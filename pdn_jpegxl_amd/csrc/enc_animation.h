// Animation encode: what a frame of an animation covers and what its header says, decided on the host from the
// change extents - or, for several rectangles per frame, the tile change map - that enc_animation_kernels.hip measures.  Host-only
// and stated once: the encoder (encoder.cc) and the test library
// (selftest.cc) both go through these functions.  (The one rule shared with the device - when a sample counts as changed under a
// tolerance - is at the end.)
#pragma once
#include <cstdint>
#include <vector>
#include "host_write.h"

namespace jxlhip {

// The bounding box of the samples whose bits differ between two consecutive frames, as the kernel leaves it: inclusive corners;
// nothing differs: x1 < 0 (the kernel's initial value, every byte 0xFF: x0 = y0 = -1 read as signed).
struct AnimExtent { int32_t x0, y0, x1, y1; };
inline bool AnimExtentEmpty(const AnimExtent& e) { return e.x1 < 0 || e.y1 < 0; }

struct AnimRect { int32_t x, y, w, h; };

// The slot every frame but the last is saved to, and the one a cropped frame shows around itself.  Not 0: a frame with a duration is
// saved only to another slot (animation.cc applies the same rule when it reads).
constexpr uint32_t kAnimSlot = 1;

// One source frame as the extents kernel reads it: the caller's device memory, rows `stride` bytes apart.
struct AnimFrameSrc { const uint8_t* data; int64_t stride; };

// Whether frame k is a key frame: the first, and every key_interval-th when key_interval >= 1.  Key frames cover the canvas.
inline bool AnimIsKeyFrame(int32_t k, int32_t key_interval) { return k == 0 || (key_interval >= 1 && k % key_interval == 0); }

// The rectangle frame k is written as on a canvas of w x h.  `ext`: what changed against frame k - 1 (ignored for key frames).
//  - key frames: the canvas;
//  - nothing changed: the 1 x 1 rectangle at (0, 0) - the frame is still written, with its duration;
//  - lossless: the bounding box; lossy: the box grown outwards to multiples of 8 canvas pixels and clipped to the canvas, so that
//    static content keeps its block grid.
AnimRect AnimFrameRect(int32_t k, int32_t key_interval, const AnimExtent& ext, int32_t w, int32_t h, bool lossless);

// The placement fields of frame k of n: a crop unless the rectangle covers the canvas, kReplace from slot kAnimSlot, saved to
// kAnimSlot unless it is the last frame.
EncFramePlacement AnimPlacement(int32_t k, int32_t n, const AnimRect& r, int32_t w, int32_t h, uint32_t duration);

// enc_animation_kernels.hip: the extents of the npairs = n - 1 consecutive pairs of `frames` (device array of n) into `out` (device,
// npairs, every byte 0xFF beforehand), one launch.  Rows are row_bytes bytes of pixel_bytes-byte pixels.
void LaunchAnimExtents(const AnimFrameSrc* frames, int32_t npairs, int32_t h, uint64_t row_bytes, uint32_t pixel_bytes, AnimExtent* out, void* stream);

// ---- several rectangles per frame (max_rects >= 2): a change map per 64 x 64-pixel tile instead of one box per pair

constexpr int32_t kAnimTile = 64;                    // pixels a tile is wide and high (ragged at the right and bottom edges)
constexpr uint32_t kAnimTileEmpty = 0xFFFFFFFFu;     // the word of a tile in which nothing differs
constexpr int32_t kAnimMaxRects = 16;                // the largest max_rects
constexpr int32_t kAnimMaxComponents = 64;           // more boxes than this after the closure: the frame is its one bounding box
inline uint32_t AnimTilesAcross(int32_t pixels) { return (uint32_t)(((int64_t)pixels + kAnimTile - 1) / kAnimTile); }

// A tile's word: the bytes x0, y0, x1, y1 (lowest first) of the inclusive box of the pixels of the tile of which some sample differs,
// relative to the tile's origin, each 0 .. 63; kAnimTileEmpty: none does.
inline uint32_t AnimTileWord(uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1) { return x0 | y0 << 8 | x1 << 16 | y1 << 24; }

// What changed over the whole canvas, from the tile table of a pair (AnimTilesAcross(w) x AnimTilesAcross(h) words, row-major): the value
// anim_extents_kernel leaves for the pair.
AnimExtent AnimTilesExtent(const uint32_t* tiles, int32_t w, int32_t h);

// The rectangles a frame that is no key frame is written as, from the tile table of its pair: at most max_rects (2 .. kAnimMaxRects),
// pairwise disjoint, together covering every changed pixel, in (y, x) order.  The rule (DESIGN.md §2 "Animation encode"):
//  1. no tile is non-empty: the 1 x 1 rectangle at (0, 0);
//  2. the 8-connected components of the non-empty tiles; a component's box is the union of its tiles' pixel boxes, for lossy grown to
//     multiples of 8 and clipped to the canvas as AnimFrameRect does;
//  3. closure: while two boxes share a pixel they are replaced by their bounding box;
//  4. more than kAnimMaxComponents boxes: the frame is its one bounding box (what max_rects = 1 writes);
//  5. boxes sorted by (y, x); while there are more than max_rects, or at least two and the cheapest pair costs at most merge_pixels:
//     the cheapest pair - cost = area(bounding box) - area(A) - area(B), ties to the smallest (index, index) - is replaced by its
//     bounding box, then the closure again and the order again.
std::vector<AnimRect> AnimFrameRects(const uint32_t* tiles, int32_t w, int32_t h, bool lossless, int32_t max_rects, int64_t merge_pixels);

// Why a call with these max_rects and merge_pixels is refused, in words; nullptr: it is not.
const char* AnimRectOptionsRefusal(int32_t max_rects, int32_t merge_pixels);

// enc_animation_kernels.hip: the tile tables of the npairs = n - 1 consecutive pairs of `frames` (device array of n) into `out` (device,
// npairs x AnimTilesAcross(h) x AnimTilesAcross(w) words; every word is written, nothing need be set beforehand), one launch.  Rows are
// w pixels of pixel_bytes (1 .. 16) bytes.
void LaunchAnimTiles(const AnimFrameSrc* frames, int32_t npairs, int32_t w, int32_t h, uint32_t pixel_bytes, uint32_t* out, void* stream);

// ---- a tolerance for "unchanged" (tolerance > 0): frame k is measured against the reference canvas R - the source of exactly what a
// decoder shows before frame k: frame 0, then every written rectangle copied in - not against frame k - 1 (DESIGN.md §2 "Animation
// encode").  The rule of one sample is stated here once, for the kernel, the host and the test library.

enum AnimSample : int32_t { kAnimU8 = 0, kAnimU16 = 1, kAnimF16 = 2, kAnimF32 = 3 };
inline uint32_t AnimSampleBytes(AnimSample kind) { return kind == kAnimU8 ? 1 : (kind == kAnimF32 ? 4 : 2); }

// Why a call with this tolerance is refused, in words; nullptr: it is not.
const char* AnimToleranceRefusal(float tolerance);

// What an integer sample may move by: floor(tolerance), at most the range of the widest integer sample.
__host__ __device__ inline uint32_t AnimIntTolerance(float tolerance) { return tolerance >= 65535.f ? 65535u : (uint32_t)tolerance; }

// Integer samples (the stored values; bits_per_sample plays no part): changed when |a - b| > floor(tolerance).
__host__ __device__ inline bool AnimIntChanged(uint32_t a, uint32_t b, uint32_t int_tolerance) { return (a > b ? a - b : b - a) > int_tolerance; }

// binary32 samples by their bits: unchanged when the bits are equal, or when both are finite and |a - b| <= tolerance (so +0 and -0
// are unchanged, equal NaN patterns are, NaN or an infinity against anything else is changed).
__host__ __device__ inline bool AnimFloatChanged(uint32_t a, uint32_t b, float tolerance) {
  if (a == b) return false;
  if ((a & 0x7F800000u) == 0x7F800000u || (b & 0x7F800000u) == 0x7F800000u) return true;
  float fa, fb;
  __builtin_memcpy(&fa, &a, 4);
  __builtin_memcpy(&fb, &b, 4);
  return !(__builtin_fabsf(fa - fb) <= tolerance);
}

// binary16 bits widened to binary32 bits (exact)
__host__ __device__ inline uint32_t AnimHalfBits(uint32_t h) {
  _Float16 v;
  const uint16_t b = (uint16_t)h;
  __builtin_memcpy(&v, &b, 2);
  const float f = (float)v;
  uint32_t out;
  __builtin_memcpy(&out, &f, 4);
  return out;
}

// binary16: equal bits are unchanged; otherwise the binary32 rule on the widened values
__host__ __device__ inline bool AnimHalfChanged(uint32_t a, uint32_t b, float tolerance) {
  return a != b && AnimFloatChanged(AnimHalfBits(a), AnimHalfBits(b), tolerance);
}

// One sample (its bits in the low bytes of a and b) of either kind
__host__ __device__ inline bool AnimSampleChanged(AnimSample kind, uint32_t a, uint32_t b, float tolerance) {
  if (kind == kAnimF32) return AnimFloatChanged(a, b, tolerance);
  if (kind == kAnimF16) return AnimHalfChanged(a, b, tolerance);
  return AnimIntChanged(a, b, AnimIntTolerance(tolerance));
}

// enc_animation_kernels.hip: the tile table of ONE frame (device rows `frame.stride` bytes apart, any sample-aligned base) against the
// reference canvas `ref` (device, tight rows of w pixel_bytes bytes) into `out` (device, AnimTilesAcross(h) x AnimTilesAcross(w) words, every
// word written): the words of LaunchAnimTiles, with "differs" meaning AnimSampleChanged.  pixel_bytes: channels x AnimSampleBytes(kind).
void LaunchAnimTilesTol(AnimFrameSrc frame, const uint8_t* ref, int32_t w, int32_t h, uint32_t pixel_bytes, AnimSample kind, float tolerance,
                        uint32_t* out, void* stream);

// enc_animation_kernels.hip: the pixels of `frame` inside the nrects (1 .. kAnimMaxRects) rectangles, each inside the w x h canvas, copied
// into the reference canvas `ref` (tight rows), one launch.  A key frame: the canvas as the one rectangle.
void LaunchAnimApplyRects(AnimFrameSrc frame, uint8_t* ref, int32_t w, uint32_t pixel_bytes, const AnimRect* rects, int32_t nrects, void* stream);

}  // namespace jxlhip
