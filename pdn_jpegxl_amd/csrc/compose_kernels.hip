// HIP kernel (gfx950) of layered images: the frames of an image, each decoded on its own into f32 scratch by the ordinary stages,
// are blended onto the canvas in file order, and the displayed result leaves in the output sample type (DESIGN.md §2 has the rules,
// §4 the measurements).
//
// One lane per canvas pixel.  The four reference slots of the pixel live in registers (4 slots x 4 channels), so no canvas-sized slot
// buffers exist: every frame is read once, one 16-byte load per pixel for four channels, and the canvas is written once.  The frame descriptors are uniform across
// a workgroup (scalar loads).  Un-premultiply, rounding to the output type and the orientation are fused into the store.
//
// Animations (every displayed image of a file, decoded in chunks of frames) run through the same loop: a frame that
// completes a displayed image stores the canvas as it stands, and the slots a later chunk still reads are loaded at entry from one
// buffer and stored at exit to another (ComposeImage::live_in / live_out, slots_in / slots_out).  A still has one displayed image, on its last frame, and no slot traffic.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "dev_types.h"
#include "dev_util.h"
#include "kernels.h"

namespace jxlhip {
namespace {

__device__ __forceinline__ float Clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// The four slots of a pixel as four named register quads, read and written through per-component selects: an array indexed by the
// (uniform) slot number went to scratch memory (72-80 B per lane), even behind unrolled compares (the compiler folds them back into an
// index); with selects the kernel has no scratch (57 VGPRs with the slot loads and stores of chunked animations, 51 before them).
struct Slots { float4 s0, s1, s2, s3; };
__device__ __forceinline__ float4 Sel(bool c, float4 a, float4 b) {
  return make_float4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}
__device__ __forceinline__ float4 ReadSlot(const Slots& sl, int s) {
  return Sel(s == 0, sl.s0, Sel(s == 1, sl.s1, Sel(s == 2, sl.s2, sl.s3)));
}
__device__ __forceinline__ void WriteSlot(Slots& sl, int s, float4 v) {
  sl.s0 = Sel(s == 0, v, sl.s0); sl.s1 = Sel(s == 1, v, sl.s1); sl.s2 = Sel(s == 2, v, sl.s2); sl.s3 = Sel(s == 3, v, sl.s3);
}
__device__ __forceinline__ float Lane(float4 v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }

// the frame's nch samples at (fx, fy): one 16-, 12-, 8- or 4-byte load
__device__ __forceinline__ void LoadFrame(const ComposeFrame& fr, int nch, int fx, int fy, float (&v)[4]) {
  const size_t i = (size_t)fy * fr.w + fx;
  if (nch == 4) {
    const float4 p = ((const float4*)fr.px)[i];
    v[0] = p.x; v[1] = p.y; v[2] = p.z; v[3] = p.w;
  } else if (nch == 3) {
    const float* p = fr.px + i * 3;
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = 0.f;
  } else if (nch == 2) {
    const float2 p = ((const float2*)fr.px)[i];
    v[0] = p.x; v[1] = p.y; v[2] = 0.f; v[3] = 0.f;
  } else {
    v[0] = fr.px[i]; v[1] = 0.f; v[2] = 0.f; v[3] = 0.f;
  }
}

// raw images (every frame replaces every channel): the frame's samples as its own decode wrote them in the output type, carried as bit
// patterns - the composite then only selects, and a pixel leaves exactly as the standalone decode of its frame would write it
__device__ __forceinline__ void LoadRaw(const ComposeFrame& fr, int nch, int out_bits, int fx, int fy, float (&v)[4]) {
  const size_t i = ((size_t)fy * fr.w + fx) * nch;
  const uint8_t* p = (const uint8_t*)fr.px;
  if (out_bits == 8 && nch == 4) {
    const uint32_t q = ((const uint32_t*)p)[i >> 2];
#pragma unroll
    for (int c = 0; c < 4; c++) v[c] = __uint_as_float((q >> (8 * c)) & 0xFF);
    return;
  }
#pragma unroll
  for (int c = 0; c < 4; c++) {
    uint32_t q = 0;
    if (c < nch) q = out_bits == 8 ? p[i + c] : (out_bits == 16 ? ((const uint16_t*)p)[i + c] : ((const uint32_t*)p)[i + c]);
    v[c] = __uint_as_float(q);
  }
}

// One channel: `old` from the channel's source slot, `ob` the alpha of the colour channels' source slot (for the alpha channel: its own
// old value), `a` the frame's alpha sample.
__device__ __forceinline__ float BlendSample(int mode, bool is_alpha, bool premul, bool clamp, float nw, float old, float a, float ob) {
  if (clamp) a = Clamp01(a);
  switch (mode) {
    case 0: return nw;
    case 1: return old + nw;
    case 2: {
      if (is_alpha) return a + ob * (1.f - a);
      if (premul) return nw + old * (1.f - a);
      const float A = a + ob * (1.f - a);
      return A == 0.f ? 0.f : (nw * a + old * ob * (1.f - a)) / A;
    }
    case 3: return is_alpha ? old : old + nw * a;
    default: return old * (clamp ? Clamp01(nw) : nw);
  }
}

// The sample as stored: what a displayed image holds for a pixel, as bit patterns of the output type.  Stated once, in two steps:
// compose_kernel stores these bits and compose_reduce_kernel averages them.
// Step 1: un-premultiply (as modular_out_kernel).
__device__ __forceinline__ void Unpremultiply(const ComposeImage& im, const float (&canvas)[4], int ai, float (&res)[4]) {
#pragma unroll
  for (int c = 0; c < 4; c++) res[c] = canvas[c];
  if (im.premul && ai >= 0 && !im.raw) {
    const float unmul = 1.0f / fmaxf(1.0f / 67108864.0f, Lane(make_float4(res[0], res[1], res[2], res[3]), ai));
#pragma unroll
    for (int c = 0; c < 4; c++) if (c < ai) res[c] *= unmul;
  }
}
// Step 2: a raw image carries the bits themselves; otherwise rounding half up like modular_out_kernel (not v_cvt_pk_u8_f32, which
// rounds ties to even): a layered file whose frames replace decodes to the same bytes as its frames would alone.
__device__ __forceinline__ uint32_t SampleBits(bool raw, float v, int out_bits, int out_float) {
  return raw ? __float_as_uint(v) : FloatToOutBits(v, out_bits, out_float);
}

// One displayed image leaves: the samples as stored, at the oriented position.  The frame loop calls this after every frame that
// completes a displayed image (a still: its last frame), with that image's buffer.
__device__ __forceinline__ void StoreDisplayed(const ComposeImage& im, uint8_t* out, const float (&canvas)[4], int x, int y, int ai) {
  const int w = im.w, h = im.h, nch = im.nch;
  float res[4];
  Unpremultiply(im, canvas, ai, res);
  int ox = x, oy = y, ow = w;
  switch (im.orientation) {
    case 2: ox = w - 1 - x; break;
    case 3: ox = w - 1 - x; oy = h - 1 - y; break;
    case 4: oy = h - 1 - y; break;
    case 5: ox = y; oy = x; ow = h; break;
    case 6: ox = h - 1 - y; oy = x; ow = h; break;
    case 7: ox = h - 1 - y; oy = w - 1 - x; ow = h; break;
    case 8: ox = y; oy = w - 1 - x; ow = h; break;
    default: break;
  }
  const size_t o = (size_t)oy * ow + ox;
  if (im.raw) {
    if (im.out_bits == 8 && nch == 4) {
      uint32_t px = 0;
#pragma unroll
      for (int c = 0; c < 4; c++) px |= SampleBits(true, res[c], 8, 0) << (8 * c);
      ((uint32_t*)out)[o] = px;
    } else {
#pragma unroll
      for (int c = 0; c < 4; c++)
        if (c < nch) StoreOutSample(out, o * nch + c, SampleBits(true, res[c], im.out_bits, im.out_float), im.out_bits);
    }
    return;
  }
  if (im.out_bits == 8 && nch == 4) {   // the common layout: one 4-byte store
    uint32_t px = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) px |= SampleBits(false, res[c], 8, 0) << (8 * c);
    ((uint32_t*)out)[o] = px;
  } else {
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (c < nch) StoreOutSample(out, o * nch + c, SampleBits(false, res[c], im.out_bits, im.out_float), im.out_bits);
  }
}

// A slot of pixel p in the slot buffers of a chunked animation: nch floats (one 16-byte access for four channels)
__device__ __forceinline__ float4 LoadSlot(const float* slots, size_t plane, int s, size_t p, int nch) {
  const float* q = slots + ((size_t)s * plane + p) * nch;
  if (nch == 4) return *(const float4*)q;
  if (nch == 3) return make_float4(q[0], q[1], q[2], 0.f);
  if (nch == 2) { const float2 v = *(const float2*)q; return make_float4(v.x, v.y, 0.f, 0.f); }
  return make_float4(q[0], 0.f, 0.f, 0.f);
}
__device__ __forceinline__ void StoreSlot(float* slots, size_t plane, int s, size_t p, int nch, float4 v) {
  float* q = slots + ((size_t)s * plane + p) * nch;
  if (nch == 4) *(float4*)q = v;
  else if (nch == 3) { q[0] = v.x; q[1] = v.y; q[2] = v.z; }
  else if (nch == 2) *(float2*)q = make_float2(v.x, v.y);
  else q[0] = v.x;
}

// The frame loop of one canvas pixel (x, y): the slots in registers, the slot traffic of a chunked animation, both sample routes and
// every blend mode.  show(frame, canvas) is called after each frame that completes a displayed image of the launch, in uniform control
// flow.  A lane that is not `inside` the canvas (compose_reduce_kernel's lanes past the image edge) touches no memory and walks the
// loop with zeros, so that it reaches every show call with the rest of its wavefront.  The caller hands in what is uniform per image
// (canvas width, channels, alpha index, pixels of a slot plane): computed once in front of its pixel loop, they stay in scalar registers.
template <class Show>
__device__ __forceinline__ void ComposePixel(const ComposeImage& im, const ComposeFrame* __restrict__ frames, int w, int nch, int ai, size_t plane, int x, int y, bool inside, Show&& show) {
  const size_t p = (size_t)y * w + x;
  Slots sl;
  sl.s0 = sl.s1 = sl.s2 = sl.s3 = make_float4(0.f, 0.f, 0.f, 0.f);
  // a later chunk of an animation: the slots some frame from here on reads, as the chunk before left them (uniform tests)
  if (inside) {
    if (im.live_in & 1) sl.s0 = LoadSlot(im.slots_in, plane, im.slot_plane[0], p, nch);
    if (im.live_in & 2) sl.s1 = LoadSlot(im.slots_in, plane, im.slot_plane[1], p, nch);
    if (im.live_in & 4) sl.s2 = LoadSlot(im.slots_in, plane, im.slot_plane[2], p, nch);
    if (im.live_in & 8) sl.s3 = LoadSlot(im.slots_in, plane, im.slot_plane[3], p, nch);
  }
  float res[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < im.count; k++) {
    const ComposeFrame& fr = frames[im.first + k];
    const float4 oc = ReadSlot(sl, fr.source[0]), oa = ReadSlot(sl, fr.source[1]);
    const float old_c[4] = {oc.x, oc.y, oc.z, oc.w}, old_a[4] = {oa.x, oa.y, oa.z, oa.w};
    const int fx = x - fr.x0, fy = y - fr.y0;
    if (inside && fx >= 0 && fy >= 0 && fx < fr.w && fy < fr.h) {
      float nw[4];
      if (im.raw) LoadRaw(fr, nch, im.out_bits, fx, fy, nw);
      else LoadFrame(fr, nch, fx, fy, nw);
      const float a = ai >= 0 ? Lane(make_float4(nw[0], nw[1], nw[2], nw[3]), ai) : 1.f;
      const float ob_c = Lane(oc, ai), ob_a = Lane(oa, ai);
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const bool is_alpha = c == ai;
        const int g = is_alpha ? 1 : 0;
        res[c] = c >= nch ? 0.f : BlendSample(fr.mode[g], is_alpha, im.premul != 0, fr.clamp[g] != 0, nw[c], is_alpha ? old_a[c] : old_c[c], a,
                                               is_alpha ? ob_a : ob_c);
      }
    } else {   // outside the crop: the source slot as it is
#pragma unroll
      for (int c = 0; c < 4; c++) res[c] = c == ai ? old_a[c] : old_c[c];
    }
    if (fr.save >= 0) WriteSlot(sl, fr.save, make_float4(res[0], res[1], res[2], res[3]));
    if (fr.show >= 0) show(fr, res);
  }
  if (inside) {
    if (im.live_out & 1) StoreSlot(im.slots_out, plane, im.slot_plane[0], p, nch, sl.s0);
    if (im.live_out & 2) StoreSlot(im.slots_out, plane, im.slot_plane[1], p, nch, sl.s1);
    if (im.live_out & 4) StoreSlot(im.slots_out, plane, im.slot_plane[2], p, nch, sl.s2);
    if (im.live_out & 8) StoreSlot(im.slots_out, plane, im.slot_plane[3], p, nch, sl.s3);
  }
}

__global__ void compose_kernel(const ComposeImage* __restrict__ imgs, const ComposeFrame* __restrict__ frames) {
  const ComposeImage& im = imgs[blockIdx.y];
  const int w = im.w, h = im.h, nch = im.nch;
  const int ai = im.has_alpha ? im.nch - 1 : -1;
  const size_t plane = (size_t)w * h;
  // a workgroup per 256-pixel row segment, one pixel per lane: the segment's row and column come from one uniform (scalar) division per
  // workgroup, none per pixel, and a wavefront's crop tests are on one row segment
  const int xseg = (w + (int)blockDim.x - 1) / (int)blockDim.x;
  for (int t = blockIdx.x; t < xseg * h; t += gridDim.x) {
    const int y = t / xseg, x = (t - y * xseg) * (int)blockDim.x + (int)threadIdx.x;
    if (x >= w) continue;
    ComposePixel(im, frames, w, nch, ai, plane, x, y, true, [=, &im](const ComposeFrame& fr, const float (&canvas)[4]) {
      StoreDisplayed(im, im.out + (size_t)fr.show * im.out_stride, canvas, x, y, ai);
    });
  }
}

// The mean of one 8 x 8 cell of a displayed image, one lane per pixel of the cell (lane l at (l & 7, l >> 3)): the samples as stored,
// summed across the wavefront in butterfly steps (every lane takes part in every step; a lane past the image edge adds nothing), and
// lane 0 stores the nch (<= 4) means at samples first, first + 1, ... of `out`.  n: the pixels of the cell that exist.  Integer samples: (sum + n / 2) / n in 32 bits; binary16 and
// binary32: the float32 sum in the butterfly's order, divided by n, rounded to the output type.
__device__ __forceinline__ void StoreCellMean(const uint32_t (&bits)[4], bool inside, int n, int nch, int out_bits, int out_float, uint8_t* out, size_t first) {
  const int lane = (int)(threadIdx.x & 63);
#pragma unroll
  for (int c = 0; c < 4; c++) {
    if (c >= nch) break;
    uint32_t mean;
    if (out_float) {
      float v = 0.f;
      if (inside) v = out_bits == 32 ? __uint_as_float(bits[c]) : __half2float(__ushort_as_half((unsigned short)bits[c]));
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
      mean = FloatToOutBits(v / (float)n, out_bits, 1);
    } else {
      uint32_t v = inside ? bits[c] : 0u;
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
      mean = (v + (uint32_t)n / 2) / (uint32_t)n;
    }
    if (lane == 0) StoreOutSample(out, first + c, mean, out_bits);
  }
}

// Thumbnails of an animation's displayed images (jxlhip_animation_next_reduced): compose_kernel's frame loop, with one wavefront per
// 8 x 8 cell of the DISPLAYED image.  The lane's canvas pixel is the inverse of the orientation, so a cell's lanes are an 8 x 8 block
// of the canvas too (mirrored or transposed), and partial cells lie at the canvas edge the orientation maps to the right / bottom.
// Slots travel at full resolution; nothing of a displayed image is stored but its cell means, out_stride bytes apart.
__global__ void compose_reduce_kernel(const ComposeImage* __restrict__ imgs, const ComposeFrame* __restrict__ frames) {
  const ComposeImage& im = imgs[blockIdx.y];
  const int w = im.w, h = im.h, nch = im.nch;
  const int ai = im.has_alpha ? nch - 1 : -1;
  const size_t plane = (size_t)w * h;
  const bool transposed = im.orientation >= 5;
  const int dw = transposed ? h : w, dh = transposed ? w : h;
  const int cw = (dw + 7) >> 3, ch = (dh + 7) >> 3;
  const int waves = (int)blockDim.x >> 6, wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  for (int t = (int)blockIdx.x * waves + wave; t < cw * ch; t += (int)gridDim.x * waves) {   // (uniform in a wavefront)
    const int cy = t / cw, cx = t - cy * cw;
    const int ox = cx * 8 + (lane & 7), oy = cy * 8 + (lane >> 3);
    const bool inside = ox < dw && oy < dh;
    const int n = min(8, dw - cx * 8) * min(8, dh - cy * 8);
    int x = ox, y = oy;
    switch (im.orientation) {   // the inverse of StoreDisplayed's mapping
      case 2: x = w - 1 - ox; break;
      case 3: x = w - 1 - ox; y = h - 1 - oy; break;
      case 4: y = h - 1 - oy; break;
      case 5: x = oy; y = ox; break;
      case 6: x = oy; y = h - 1 - ox; break;
      case 7: x = w - 1 - oy; y = h - 1 - ox; break;
      case 8: x = w - 1 - oy; y = ox; break;
      default: break;
    }
    ComposePixel(im, frames, w, nch, ai, plane, x, y, inside, [&](const ComposeFrame& fr, const float (&canvas)[4]) {
      const int j = fr.show;
      float res[4];
      Unpremultiply(im, canvas, ai, res);
      uint32_t bits[4];
#pragma unroll
      for (int c = 0; c < 4; c++) bits[c] = SampleBits(im.raw != 0, res[c], im.out_bits, im.out_float);
      StoreCellMean(bits, inside, n, nch, im.out_bits, im.out_float, im.out + (size_t)j * im.out_stride, (size_t)t * nch);
    });
  }
}

// The same cell means of one displayed image that is in memory already (a file that is one single-frame image: the ordinary decode
// wrote it, oriented, to scratch): dw x dh pixels of nch samples, four channels at a time (a CMYK image with alpha has five).
__global__ void reduce_displayed_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int dw, int dh, int nch, int out_bits, int out_float) {
  const int cw = (dw + 7) >> 3, ch = (dh + 7) >> 3;
  const int waves = (int)blockDim.x >> 6, wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  for (int t = (int)blockIdx.x * waves + wave; t < cw * ch; t += (int)gridDim.x * waves) {
    const int cy = t / cw, cx = t - cy * cw;
    const int ox = cx * 8 + (lane & 7), oy = cy * 8 + (lane >> 3);
    const bool inside = ox < dw && oy < dh;
    const int n = min(8, dw - cx * 8) * min(8, dh - cy * 8);
    for (int c0 = 0; c0 < nch; c0 += 4) {   // (uniform)
      uint32_t bits[4] = {0, 0, 0, 0};
      if (inside) {
        const size_t i = ((size_t)oy * dw + ox) * nch + c0;
#pragma unroll
        for (int c = 0; c < 4; c++)
          if (c0 + c < nch) bits[c] = out_bits == 8 ? src[i + c] : (out_bits == 16 ? ((const uint16_t*)src)[i + c] : ((const uint32_t*)src)[i + c]);
      }
      StoreCellMean(bits, inside, n, min(4, nch - c0), out_bits, out_float, dst, (size_t)t * nch + c0);
    }
  }
}

}  // namespace

void LaunchCompose(const ComposeImage* imgs, const ComposeFrame* frames, int nimg, int max_segments, hipStream_t s) {
  if (nimg <= 0) return;
  const unsigned blocks = (unsigned)std::max(1, std::min(1 << 20, max_segments));
  hipLaunchKernelGGL(compose_kernel, dim3(blocks, nimg), dim3(256), 0, s, imgs, frames);
}

void LaunchComposeReduce(const ComposeImage* imgs, const ComposeFrame* frames, int nimg, int max_cells, hipStream_t s) {
  if (nimg <= 0) return;
  const unsigned blocks = (unsigned)std::max(1, std::min(1 << 20, (max_cells + 3) / 4));   // four wavefronts, a cell each
  hipLaunchKernelGGL(compose_reduce_kernel, dim3(blocks, nimg), dim3(256), 0, s, imgs, frames);
}

void LaunchReduceDisplayed(const uint8_t* src, uint8_t* dst, int dw, int dh, int nch, int out_bits, int out_float, hipStream_t s) {
  const int cells = ((dw + 7) / 8) * ((dh + 7) / 8);
  const unsigned blocks = (unsigned)std::max(1, std::min(1 << 20, (cells + 3) / 4));
  hipLaunchKernelGGL(reduce_displayed_kernel, dim3(blocks), dim3(256), 0, s, src, dst, dw, dh, nch, out_bits, out_float);
}

}  // namespace jxlhip
