// Device helpers shared by the encoder's kernel files (encode_kernels.hip, lossless_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "modular_rules.h"   // PackSigned, the predictors and the neighbourhood, as the decoder has them

namespace jxlhip {

// hybrid-uint token of `v` under the config (split_exponent 4, msb_in_token 2, lsb_in_token 0)
__device__ __forceinline__ void HybridD(uint32_t v, uint32_t* tok, uint32_t* nbits, uint32_t* bits) {
  if (v < 16) { *tok = v; *nbits = 0; *bits = 0; return; }
  const uint32_t n = 31 - __clz(v), m = v - (1u << n);
  *tok = 16 + ((n - 4) << 2) + (m >> (n - 2));
  *nbits = n - 2;
  *bits = m & ((1u << (n - 2)) - 1);
}

}  // namespace jxlhip
