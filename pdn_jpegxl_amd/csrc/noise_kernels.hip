// HIP kernels (gfx950) of synthetic noise on lossy frames (frame flag 1; DESIGN.md §2 has the rules, §4.9 the measurements).
//
// noise_generate_kernel: the three random planes R_k.  A 256x256 group is one generator of eight xorshift128+ lanes whose 16 values
// per step fill the group's rows plane by plane, so a group is a chain of 3 * gh * ceil(gw / 16) dependent steps (12 288 for a full
// group).  One hardware lane per generator lane, eight per group, eight groups per wavefront, every group of every noise frame of the
// launch side by side: the launch lasts as long as one group's chain.  Per step a lane stores its two values (8 lanes: 64 contiguous
// bytes of a row).
//
// noise_convolve_kernel: N_k = 0.22 * (0.16 * sum over the 5x5 window of R_k - 4 * R_k), mirrored at the frame edge like the loop
// filters.  The values of R_k are 1 + m * 2^-23 with integer m < 2^23 and the weights sum to zero, so N_k = (4 * sum(m) - 100 * m_centre)
// * (0.22 / 25) * 2^-23: the window is summed in integers, exactly and in any order (a band convolves to the same bits as the whole
// frame), and rounded twice at the end.  64x16 output tiles with a 2-pixel halo in LDS, separable 5-sums.
//
// The addition to X, Y, B is part of the output phase of the filter kernels (tile_kernels.hip, AddNoise).
#include <hip/hip_runtime.h>
#include <algorithm>
#include "dev_types.h"
#include "dev_util.h"
#include "kernels.h"

namespace jxlhip {
namespace {

__device__ __forceinline__ uint64_t SplitMix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ float BitsToUnitFloat(uint32_t v) { return __uint_as_float((v >> 9) | 0x3F800000u); }   // [1, 2)

constexpr int kGenLanes = 8;      // xorshift lanes of a generator
constexpr int kGenThreads = 64;   // a wavefront: eight groups

__global__ __launch_bounds__(kGenThreads) void noise_generate_kernel(const DevImage* __restrict__ imgs) {
  const DevImage& im = imgs[blockIdx.y];
  if (!im.has_noise) return;
  const int t = blockIdx.x * kGenThreads + threadIdx.x;
  const int g = t / kGenLanes, lane = t % kGenLanes;
  const int xg = im.xg;
  if (g >= (im.noise_gy1 - im.noise_gy0) * xg) return;
  const int x0 = (g % xg) * kGroupDim, y0 = (im.noise_gy0 + g / xg) * kGroupDim;
  const int gw = min(kGroupDim, im.w - x0), gh = min(kGroupDim, im.h - y0);   // > 0: the group lies in the frame
  // lane i of the generator is i SplitMix64 steps behind lane 0's seed
  uint64_t s0 = SplitMix64((((uint64_t)im.noise_seed[0] << 32) + im.noise_seed[1]) + 0x9E3779B97F4A7C15ull);
  uint64_t s1 = SplitMix64((((uint64_t)(uint32_t)x0 << 32) + (uint32_t)y0) + 0x9E3779B97F4A7C15ull);
  for (int i = 0; i < lane; i++) { s0 = SplitMix64(s0); s1 = SplitMix64(s1); }
  const int batches = (gw + 15) / 16;
  const int xl = 2 * lane;   // this lane's two columns of a batch of 16
  for (int k = 0; k < 3; k++) {
    float* row = im.noise_rnd[k] + (size_t)y0 * im.w + x0;
    for (int y = 0; y < gh; y++, row += im.w) {
      for (int b = 0; b < batches; b++) {
        uint64_t a = s0;
        const uint64_t c = s1, out = a + c;
        s0 = c;
        a ^= a << 23;
        a ^= c ^ (a >> 18) ^ (c >> 5);
        s1 = a;
        const int x = b * 16 + xl;   // (the tail of a row's last batch is dropped)
        if (x < gw) row[x] = BitsToUnitFloat((uint32_t)out);
        if (x + 1 < gw) row[x + 1] = BitsToUnitFloat((uint32_t)(out >> 32));
      }
    }
  }
}

constexpr int kConvW = 64, kConvH = 16;

__global__ __launch_bounds__(256) void noise_convolve_kernel(const DevImage* __restrict__ imgs) {
  __shared__ int32_t m[kConvH + 4][kConvW + 4];   // mantissas of the tile and its halo
  __shared__ int32_t hs[kConvH + 4][kConvW];      // horizontal 5-sums
  const DevImage& im = imgs[blockIdx.z];
  if (!im.has_noise) return;
  const int w = im.w, h = im.h;
  const int tiles_x = (w + kConvW - 1) / kConvW;
  const int band_h = im.band_y1 - im.band_y0;
  if ((int)blockIdx.x >= tiles_x * ((band_h + kConvH - 1) / kConvH)) return;
  const int x0 = ((int)blockIdx.x % tiles_x) * kConvW, y0 = im.band_y0 + ((int)blockIdx.x / tiles_x) * kConvH;
  const float* __restrict__ rnd = im.noise_rnd[blockIdx.y];
  // rows y0 - 2 .. y0 + 17 mirrored into the frame: they lie in the generated group rows (a band starts and ends on a group row)
  for (int e = threadIdx.x; e < (kConvH + 4) * (kConvW + 4); e += 256) {
    const int ly = e / (kConvW + 4), lx = e % (kConvW + 4);
    const size_t at = (size_t)ReflectIndex(y0 - 2 + ly, h) * w + ReflectIndex(x0 - 2 + lx, w);
    m[ly][lx] = (int32_t)(__float_as_uint(rnd[at]) & 0x7FFFFFu);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < (kConvH + 4) * kConvW; e += 256) {
    const int ly = e / kConvW, lx = e % kConvW;
    hs[ly][lx] = m[ly][lx] + m[ly][lx + 1] + m[ly][lx + 2] + m[ly][lx + 3] + m[ly][lx + 4];
  }
  __syncthreads();
  float* __restrict__ dst = im.noise[blockIdx.y];
  for (int e = threadIdx.x; e < kConvH * kConvW; e += 256) {
    const int ly = e / kConvW, lx = e % kConvW;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= w || y >= im.band_y1) continue;
    const int32_t sum = hs[ly][lx] + hs[ly + 1][lx] + hs[ly + 2][lx] + hs[ly + 3][lx] + hs[ly + 4][lx];   // < 25 * 2^23
    const int32_t num = 4 * sum - 100 * m[ly + 2][lx + 2];                                                // |num| < 2^30
    dst[(size_t)y * w + x] = (float)num * (0.22f / 25.0f / 8388608.0f);
  }
}

}  // namespace

void LaunchNoise(const DevImage* imgs, int nimg, int max_groups, int max_w, int max_h, hipStream_t s) {
  const int gen_threads = max_groups * kGenLanes;
  hipLaunchKernelGGL(noise_generate_kernel, dim3((gen_threads + kGenThreads - 1) / kGenThreads, nimg), dim3(kGenThreads), 0, s, imgs);
  const int tiles = ((max_w + kConvW - 1) / kConvW) * ((max_h + kConvH - 1) / kConvH);
  hipLaunchKernelGGL(noise_convolve_kernel, dim3(tiles, 3, nimg), dim3(256), 0, s, imgs);
}

}  // namespace jxlhip
