// Animation encode: what a frame of an animation covers and what its header says, decided on the host from the
// change extents that enc_animation_kernels.hip measures.  Host-only and stated once: the encoder (encoder.cc) and the test library
// (selftest.cc) both go through these functions.
#pragma once
#include <cstdint>
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

}  // namespace jxlhip
