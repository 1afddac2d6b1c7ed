// Device helpers shared by the encoder's kernel files (encode_kernels.hip, lossless_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace jxlhip {

__device__ __forceinline__ uint32_t PackSignedD(int32_t v) { return v >= 0 ? (uint32_t)v << 1 : (((uint32_t)(-(int64_t)v)) << 1) - 1; }
// hybrid-uint token of `v` under the config (split_exponent 4, msb_in_token 2, lsb_in_token 0)
__device__ __forceinline__ void HybridD(uint32_t v, uint32_t* tok, uint32_t* nbits, uint32_t* bits) {
  if (v < 16) { *tok = v; *nbits = 0; *bits = 0; return; }
  const uint32_t n = 31 - __clz(v), m = v - (1u << n);
  *tok = 16 + ((n - 4) << 2) + (m >> (n - 2));
  *nbits = n - 2;
  *bits = m & ((1u << (n - 2)) - 1);
}
__device__ __forceinline__ int32_t GradientPred(int32_t W, int32_t N, int32_t NW) {
  const int64_t mn = W < N ? W : N, mx = W < N ? N : W, gr = (int64_t)W + N - NW;
  return (int32_t)(gr < mn ? mn : (gr > mx ? mx : gr));
}

}  // namespace jxlhip
