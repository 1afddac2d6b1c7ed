// Cell means for the reduced-size decode (decoder option "downscale" = 8, DESIGN.md §2, rules 2 and 3).
//
//   alpha_reduce_kernel   VarDCT frames with alpha: the mean of every 8x8 cell of the alpha plane (samples of the output type, as
//                         alpha_finish_kernel leaves them) -> DevImage::ds_alpha, which lf_output_kernel (tile_kernels.hip) merges.
//   box_reduce_kernel     Modular frames: the mean of every 8x8 cell of the full-size interleaved output samples (1..5 channels of
//                         1 / 2 / 4 bytes, after every inverse transform, CMYK inversion and un-premultiplication) -> the caller's
//                         buffer, at the oriented position.
//
// A lane owns one cell; neighbouring lanes own neighbouring cells of a cell row, so a wavefront reads 64 x 8 contiguous pixels per
// row of its cells.  A cell at the right / bottom edge holds (w - 8 cx) x (h - 8 cy) pixels when that is less: the loops run over
// the pixels that exist, nothing is padded.  Integer samples: (sum + n / 2) / n in 32-bit arithmetic (64 x 65535 fits); float
// samples: the sum in f32 in row order, one division.  All images of a launch side by side (grid.y = image).
#include <hip/hip_runtime.h>
#include <algorithm>
#include "dev_types.h"
#include "dev_util.h"
#include "kernels.h"

namespace jxlhip {

namespace {

__device__ __forceinline__ uint32_t ByteSum(uint32_t v) {   // sum of the four bytes of v
  const uint32_t t = (v & 0x00FF00FFu) + ((v >> 8) & 0x00FF00FFu);
  return (t & 0xFFFFu) + (t >> 16);
}
__device__ __forceinline__ uint32_t HalfSum(uint32_t v) { return (v & 0xFFFFu) + (v >> 16); }
__device__ __forceinline__ float HalfBitsToFloat(uint16_t v) { return __half2float(__ushort_as_half(v)); }
__device__ __forceinline__ uint16_t FloatToHalfBits(float f) { return __half_as_ushort(__float2half_rn(f)); }

}  // namespace

__global__ __launch_bounds__(256) void alpha_reduce_kernel(const DevImage* __restrict__ imgs) {
  const DevImage& im = imgs[blockIdx.y];
  if (!im.ds || im.is_modular || !im.has_alpha) return;
  const int w = im.w, h = im.h, cw = im.ds_w;
  const size_t n = (size_t)cw * im.ds_h;
  const bool whole = (w & 7) == 0;   // every cell is 8 samples wide and starts on an 8-sample boundary of its (256-byte aligned) plane
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int cx = (int)(i % (size_t)cw), cy = (int)(i / (size_t)cw);
    const int nx = min(8, w - 8 * cx), ny = min(8, h - 8 * cy);
    const size_t base = (size_t)cy * 8 * w + (size_t)cx * 8;
    const uint32_t cnt = (uint32_t)(nx * ny);
    if (im.out_float) {
      float sum = 0.f;
      if (im.out_bits == 32) {
        const float* p = (const float*)im.alpha + base;
        for (int r = 0; r < ny; r++)
          for (int x = 0; x < nx; x++) sum += p[(size_t)r * w + x];
        ((float*)im.ds_alpha)[i] = sum / (float)cnt;
      } else {
        const uint16_t* p = (const uint16_t*)im.alpha + base;
        for (int r = 0; r < ny; r++)
          for (int x = 0; x < nx; x++) sum += HalfBitsToFloat(p[(size_t)r * w + x]);
        ((uint16_t*)im.ds_alpha)[i] = FloatToHalfBits(sum / (float)cnt);
      }
      continue;
    }
    uint32_t sum = 0;
    if (im.out_bits == 8) {
      const uint8_t* p = im.alpha + base;
      if (whole) {   // one 8-byte load per row: a wavefront reads 512 contiguous bytes
        for (int r = 0; r < ny; r++) {
          const uint2 v = *(const uint2*)(p + (size_t)r * w);
          sum += ByteSum(v.x) + ByteSum(v.y);
        }
      } else {
        for (int r = 0; r < ny; r++)
          for (int x = 0; x < nx; x++) sum += p[(size_t)r * w + x];
      }
      im.ds_alpha[i] = (uint8_t)((sum + cnt / 2) / cnt);
    } else {
      const uint16_t* p = (const uint16_t*)im.alpha + base;
      if (whole) {   // one 16-byte load per row
        for (int r = 0; r < ny; r++) {
          const uint4 v = *(const uint4*)(p + (size_t)r * w);
          sum += HalfSum(v.x) + HalfSum(v.y) + HalfSum(v.z) + HalfSum(v.w);
        }
      } else {
        for (int r = 0; r < ny; r++)
          for (int x = 0; x < nx; x++) sum += p[(size_t)r * w + x];
      }
      ((uint16_t*)im.ds_alpha)[i] = (uint16_t)((sum + cnt / 2) / cnt);
    }
  }
}

namespace {

// One cell of an image of interleaved samples of type T (kFloat: binary32 as float, binary16 as its bit pattern in uint16_t).  The
// channel loops have a constant bound so that the five sums stay in registers.
template <typename T, bool kFloat>
__device__ __forceinline__ void BoxReduceCell(const DevImage& im, int cx, int cy) {
  const int w = im.w, h = im.h, nch = im.nch_out;
  const int nx = min(8, w - 8 * cx), ny = min(8, h - 8 * cy);
  const uint32_t cnt = (uint32_t)(nx * ny);
  const T* src = (const T*)im.out + ((size_t)cy * 8 * w + (size_t)cx * 8) * nch;
  T* dst = (T*)im.ds_out + OrientedIndex(im.ds_orient, cx, cy, im.ds_w, im.ds_h) * nch;
  if (kFloat) {
    float sum[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < ny; r++) {
      const T* row = src + (size_t)r * w * nch;
      for (int x = 0; x < nx; x++) {
#pragma unroll
        for (int c = 0; c < 5; c++)
          if (c < nch) sum[c] += sizeof(T) == 4 ? __uint_as_float((uint32_t)row[x * nch + c]) : HalfBitsToFloat((uint16_t)row[x * nch + c]);
      }
    }
#pragma unroll
    for (int c = 0; c < 5; c++)
      if (c < nch) {
        const float m = sum[c] / (float)cnt;
        dst[c] = sizeof(T) == 4 ? (T)__float_as_uint(m) : (T)FloatToHalfBits(m);
      }
  } else {
    uint32_t sum[5] = {0, 0, 0, 0, 0};
    for (int r = 0; r < ny; r++) {
      const T* row = src + (size_t)r * w * nch;
      for (int x = 0; x < nx; x++) {
#pragma unroll
        for (int c = 0; c < 5; c++)
          if (c < nch) sum[c] += row[x * nch + c];
      }
    }
#pragma unroll
    for (int c = 0; c < 5; c++)
      if (c < nch) dst[c] = (T)((sum[c] + cnt / 2) / cnt);
  }
}

}  // namespace

__global__ __launch_bounds__(256) void box_reduce_kernel(const DevImage* __restrict__ imgs) {
  const DevImage& im = imgs[blockIdx.y];
  if (!im.ds || !im.is_modular) return;
  const int cw = im.ds_w;
  const size_t n = (size_t)cw * im.ds_h;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int cx = (int)(i % (size_t)cw), cy = (int)(i / (size_t)cw);
    if (im.out_bits == 8) BoxReduceCell<uint8_t, false>(im, cx, cy);
    else if (im.out_bits == 16 && !im.out_float) BoxReduceCell<uint16_t, false>(im, cx, cy);
    else if (im.out_bits == 16) BoxReduceCell<uint16_t, true>(im, cx, cy);
    else BoxReduceCell<uint32_t, true>(im, cx, cy);
  }
}

static unsigned CellBlocks(size_t max_cells) { return (unsigned)std::max<size_t>(1, std::min<size_t>((max_cells + 255) / 256, 2048)); }

void LaunchAlphaReduce(const DevImage* imgs, int nimg, size_t max_cells, hipStream_t s) {
  if (nimg <= 0) return;
  hipLaunchKernelGGL(alpha_reduce_kernel, dim3(CellBlocks(max_cells), nimg), dim3(256), 0, s, imgs);
}

void LaunchBoxReduce(const DevImage* imgs, int nimg, size_t max_cells, hipStream_t s) {
  if (nimg <= 0) return;
  hipLaunchKernelGGL(box_reduce_kernel, dim3(CellBlocks(max_cells), nimg), dim3(256), 0, s, imgs);
}

}  // namespace jxlhip
