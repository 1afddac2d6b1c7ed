// HIP kernels (gfx950) of the distance map and of the closed quantisation loop of efforts 8 and 9 ("Distance map: rules
// of this project", and §4.10).  This map is this project's own measure in the XYB domain.  It is NOT Butteraugli.
//
//   dist_mask_kernel      M = 1 / (1 + B5(|O_Y - B5(O_Y)|) / a0): the masking of the original, once per picture
//   dist_cell_kernel      per channel E = R - O, L = B5(B5(E)), H = E - L; P = sum_c s_c^2 (M^2 H_c^2 + L_c^2); per 8x8 cell, clipped to
//                         the frame, T = K * mean(P^2)^(1/4)
//   dist_correct_kernel   per varblock the maximum of its cells' T, r = T / tau, and the corrected quant field
//
// B5 is the separable [1 4 6 4 1] / 16, rows first.  Beyond the frame it reads the mirrored sample by ReflectIndex, which repeats the
// reflection until the index is inside.  The extended plane is symmetric about every edge and so is the kernel, hence the blur of the
// extended plane at an outside position equals the blur at the mirrored inside position: a tile loads its halo through ReflectIndex
// once and both nested blurs run on the tile alone.  64x16 output tiles, 4-pixel halo, LDS (the pattern of noise_convolve_kernel).
//
// Every sum has a fixed order (a thread per cell row, then a thread per cell): the results do not depend on the launch order, no
// atomics.
#include <hip/hip_runtime.h>
#include "dev_util.h"
#include "enc_types.h"
#include "varblock_rules.h"

namespace jxlhip {
namespace {

constexpr int kTW = 64, kTH = 16;          // output tile
constexpr int kInW = kTW + 8, kInH = kTH + 8;   // with the halo of two nested blurs
constexpr int kMidW = kTW + 4, kMidH = kTH + 4; // after the first blur

// out[(ih - 4) x (iw - 4)] = B5(in[ih x iw]); tmp holds ih x (iw - 4).  All in LDS, rows tight.  Ends with a barrier.
__device__ __forceinline__ void Blur5(const float* in, int ih, int iw, float* tmp, float* out) {
  const int ow = iw - 4, oh = ih - 4;
  for (int e = threadIdx.x; e < ih * ow; e += 256) {
    const int y = e / ow, x = e % ow;
    const float* p = in + y * iw + x;
    tmp[e] = (p[0] + p[4] + 4.0f * (p[1] + p[3]) + 6.0f * p[2]) * (1.0f / 16.0f);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < oh * ow; e += 256) {
    const int y = e / ow, x = e % ow;
    const float* p = tmp + y * ow + x;
    out[e] = (p[0] + p[4 * ow] + 4.0f * (p[ow] + p[3 * ow]) + 6.0f * p[2 * ow]) * (1.0f / 16.0f);
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void dist_mask_kernel(DistMap dm) {
  __shared__ float a[kInH * kInW], t[kInH * kMidW], b[kMidH * kMidW];
  const int tiles_x = (dm.w + kTW - 1) / kTW;
  const int x0 = ((int)blockIdx.x % tiles_x) * kTW, y0 = ((int)blockIdx.x / tiles_x) * kTH;
  const float* __restrict__ oy = dm.orig[1];
  for (int e = threadIdx.x; e < kInH * kInW; e += 256) {
    const int ly = e / kInW, lx = e % kInW;
    a[e] = oy[(size_t)ReflectIndex(y0 - 4 + ly, dm.h) * dm.w + ReflectIndex(x0 - 4 + lx, dm.w)];
  }
  __syncthreads();
  Blur5(a, kInH, kInW, t, b);
  for (int e = threadIdx.x; e < kMidH * kMidW; e += 256) {
    const int ly = e / kMidW, lx = e % kMidW;
    b[e] = fabsf(a[(ly + 2) * kInW + lx + 2] - b[e]);
  }
  __syncthreads();
  Blur5(b, kMidH, kMidW, t, a);   // a: kTH x kTW
  for (int e = threadIdx.x; e < kTH * kTW; e += 256) {
    const int x = x0 + e % kTW, y = y0 + e / kTW;
    if (x < dm.w && y < dm.h) dm.mask[(size_t)y * dm.w + x] = 1.0f / (1.0f + a[e] / dm.a0);
  }
}

__global__ __launch_bounds__(256) void dist_cell_kernel(DistMap dm) {
  __shared__ float a[kInH * kInW], t[kInH * kMidW], b[kMidH * kMidW];
  __shared__ float rows[kTH * (kTW / 8)];   // sums of P^2 over the 8 pixels of a cell row
  const int tiles_x = (dm.w + kTW - 1) / kTW;
  const int x0 = ((int)blockIdx.x % tiles_x) * kTW, y0 = ((int)blockIdx.x / tiles_x) * kTH;
  // a thread owns pixels e = threadIdx.x + 256 * k of the tile
  float p[4] = {0.f, 0.f, 0.f, 0.f}, m2[4];
  for (int k = 0; k < 4; k++) {
    const int e = threadIdx.x + 256 * k;
    const int x = min(x0 + e % kTW, dm.w - 1), y = min(y0 + e / kTW, dm.h - 1);
    const float m = dm.mask[(size_t)y * dm.w + x];
    m2[k] = m * m;
  }
  for (int c = 0; c < 3; c++) {
    const float* __restrict__ o = dm.orig[c];
    const float* __restrict__ r = dm.recon[c];
    for (int e = threadIdx.x; e < kInH * kInW; e += 256) {
      const int ly = e / kInW, lx = e % kInW;
      const int y = ReflectIndex(y0 - 4 + ly, dm.h), x = ReflectIndex(x0 - 4 + lx, dm.w);
      a[e] = r[(size_t)y * dm.recon_stride + x] - o[(size_t)y * dm.w + x];
    }
    __syncthreads();
    float err[4];
    for (int k = 0; k < 4; k++) {
      const int e = threadIdx.x + 256 * k;
      err[k] = a[(e / kTW + 4) * kInW + e % kTW + 4];
    }
    Blur5(a, kInH, kInW, t, b);
    Blur5(b, kMidH, kMidW, t, a);   // a: L on the tile (every thread has read its err[] before the first barrier inside Blur5)
    const float s2 = dm.s2[c];
    for (int k = 0; k < 4; k++) {
      const float l = a[threadIdx.x + 256 * k], hgh = err[k] - l;
      p[k] += s2 * (m2[k] * hgh * hgh + l * l);
    }
    __syncthreads();
  }
  for (int k = 0; k < 4; k++) a[threadIdx.x + 256 * k] = p[k] * p[k];
  __syncthreads();
  // cells of the tile: 8 across, 2 down; a thread per (pixel row, cell column), then a thread per cell, both in a fixed order
  if (threadIdx.x < kTH * (kTW / 8)) {
    const int ly = threadIdx.x / (kTW / 8), cx = threadIdx.x % (kTW / 8);
    float sum = 0.f;
    if (y0 + ly < dm.h)
      for (int i = 0; i < 8; i++)
        if (x0 + cx * 8 + i < dm.w) sum += a[ly * kTW + cx * 8 + i];
    rows[threadIdx.x] = sum;
  }
  __syncthreads();
  if (threadIdx.x < (kTH / 8) * (kTW / 8)) {
    const int cy = threadIdx.x / (kTW / 8), cx = threadIdx.x % (kTW / 8);
    const int bx = x0 / 8 + cx, by = y0 / 8 + cy;
    if (bx < dm.w8 && by < dm.h8) {
      float sum = 0.f;
      for (int i = 0; i < 8; i++) sum += rows[(cy * 8 + i) * (kTW / 8) + cx];
      const int n = min(8, dm.w - bx * 8) * min(8, dm.h - by * 8);
      dm.cell[(size_t)by * dm.w8 + bx] = dm.k * sqrtf(sqrtf(sum / (float)n));
    }
  }
}

// One thread per cell; the thread of a varblock's first cell takes the maximum of its cells' distances and writes the corrected quant
// field to every cell it covers (no other thread writes them).
__global__ void dist_correct_kernel(EncImage im, const float* __restrict__ cell, const int32_t* __restrict__ q0, float tau, float p_up,
                                    float p_down, int allow_down) {
  const int ncell = im.w8 * im.h8;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ncell || !(tau > 0.f)) return;
  const uint32_t st = im.strat[i];
  if (!(st & 0x80)) return;
  const int cx = 1 << StrategyLog2Cx(st & 0x7F), cy = 1 << StrategyLog2Cy(st & 0x7F);
  float tv = 0.f;
  for (int y = 0; y < cy; y++)
    for (int x = 0; x < cx; x++) tv = fmaxf(tv, cell[i + y * im.w8 + x]);
  const float r = tv / tau;
  const int32_t q = im.rawq[i], base = q0[i];
  float f = (float)q;
  if (r > 1.f) f *= powf(r, p_up);
  else if (r < 1.f && allow_down) f *= powf(fmaxf(r, 1e-3f), p_down);
  else return;
  const int32_t lo = max(1, (base + 1) / 2), hi = min(256, 4 * base);
  const int32_t qn = max(lo, min(hi, (int32_t)rintf(f)));
  for (int y = 0; y < cy; y++)
    for (int x = 0; x < cx; x++) im.rawq[i + y * im.w8 + x] = qn;
}

}  // namespace

void LaunchDistMask(const DistMap& dm, hipStream_t s) {
  const int tiles = ((dm.w + kTW - 1) / kTW) * ((dm.h + kTH - 1) / kTH);
  hipLaunchKernelGGL(dist_mask_kernel, dim3(tiles), dim3(256), 0, s, dm);
}
void LaunchDistCells(const DistMap& dm, hipStream_t s) {
  const int tiles = ((dm.w + kTW - 1) / kTW) * ((dm.h + kTH - 1) / kTH);
  hipLaunchKernelGGL(dist_cell_kernel, dim3(tiles), dim3(256), 0, s, dm);
}
void LaunchDistCorrect(const EncImage& im, const float* cell, const int32_t* q0, float tau, float p_up, float p_down, bool allow_down, hipStream_t s) {
  const int ncell = im.w8 * im.h8;
  hipLaunchKernelGGL(dist_correct_kernel, dim3((ncell + 255) / 256), dim3(256), 0, s, im, cell, q0, tau, p_up, p_down, allow_down ? 1 : 0);
}

}  // namespace jxlhip
