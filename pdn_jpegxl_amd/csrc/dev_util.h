// Small device-side helpers shared by the kernel files (included after <hip/hip_runtime.h>).
#pragma once
#include <stdint.h>
#include <hip/hip_fp16.h>

namespace jxlhip {

// Index v reflected into [0, n), edge sample repeated (... 1 0 | 0 1 .. n-1 | n-1 n-2 ...), for any n >= 1: the reflection repeats
// until the index is inside, because a frame 1 or 2 samples across is narrower than the loop filters' reach of 3.  Every loop
// filter, the encoder's analysis and the oracle reflect by this rule; the CPU suite checks it through jxlhip_selftest_reflect.
__host__ __device__ __forceinline__ int ReflectIndex(int v, int n) {
  while (v < 0 || v >= n) v = v < 0 ? -v - 1 : 2 * n - 1 - v;
  return v;
}

// Position in the displayed image of sample (x, y) of a w x h image stored in codestream orientation, for EXIF orientation o (1..8):
// index into tight rows of w (o <= 4) or h (o >= 5) samples.  The inverse of orient_kernel's mapping (kernels.hip).
__host__ __device__ __forceinline__ size_t OrientedIndex(int o, int x, int y, int w, int h) {
  int ox, oy;
  switch (o) {
    case 2: ox = w - 1 - x; oy = y; break;
    case 3: ox = w - 1 - x; oy = h - 1 - y; break;
    case 4: ox = x; oy = h - 1 - y; break;
    case 5: ox = y; oy = x; break;
    case 6: ox = h - 1 - y; oy = x; break;
    case 7: ox = h - 1 - y; oy = w - 1 - x; break;
    case 8: ox = y; oy = w - 1 - x; break;
    default: ox = x; oy = y; break;
  }
  return (size_t)oy * (size_t)(o >= 5 ? h : w) + (size_t)ox;
}

// Context offset of the HF coefficient tokens for the predicted non-zero count nzl in [0, 63]: a step function with eight values
// (0, 31, 62, 93, 123, 152, 180, 206) and thresholds at 2, 3, 5, 9, 13, 21 and 33, computed in registers so that the batched HF
// token loop has no table lookup in front of its context-map read.  The CPU suite checks all 64 inputs through
// jxlhip_selftest_nnz_ctx.
// The thresholds are the set bits of a 64-bit word (threshold t at bit t - 1), so the thresholds still above nzl are one shift and
// a bit count, and the eight values sit in a second word in that order: six instructions, where seven comparisons with their adds
// and the wait states between them were twenty-five - on every step of the batched loop.  nzl above 63 (no valid count gives one: a
// block's non-zeros per covered cell are at most 63) is taken as 63, so that the shift is defined for every input.
__host__ __device__ __forceinline__ uint32_t NnzBucketCtx(uint32_t nzl) {
  const uint32_t above = (uint32_t)__builtin_popcountll(0x100101116ull >> (nzl < 63 ? nzl : 63));
  return (uint32_t)(0x001F3E5D7B98B4CEull >> (8 * above)) & 0xFFu;
}

// A non-zero HF coefficient leaves the token loops as the upper half of a 32-bit entry (scan position | value << 16): it must fit
// int16, and a stream with a wider one is refused (kErrRange).  Stated once for HfTakeCoeff and HfTakeToken (HfScalarRun folds the
// same bound into one OR per value); the CPU suite checks the bounds through jxlhip_selftest_hf_entry_fits.
__host__ __device__ __forceinline__ bool HfEntryFits(int32_t v) { return v == (int32_t)(int16_t)v; }

// Position context of an HF coefficient token, for ks = scan position / cells the varblock covers, in [1, 63]: the format's three pieces
// (ks - 1 below 16, then one context per two positions, from 32 on one per four) as the minimum of three lines, without branches.
// The CPU suite checks all 63 inputs against the piecewise definition through jxlhip_selftest_hf_pos_ctx.
__host__ __device__ __forceinline__ uint32_t HfPosCtx(uint32_t ks) {
  const uint32_t a = ks - 1, b = 7 + (ks >> 1), c = 15 + (ks >> 2);
  const uint32_t bc = b < c ? b : c;
  return a < bc ? a : bc;
}

// Context of a block's non-zero-count token.  The prediction: from the counts of the block above and the block to the left (each
// already divided by the cells its block covers), 32 for the group's first block.  Its bucket: clamped at 64, one context per value below
// 8 and one per two values from there on (0 .. 36).  The CPU suite checks both through jxlhip_selftest_hf_nnz_predict / _bucket.
// Both are written as selects and minima: as nested conditions they became three exec-masked regions per block start of the batched
// HF loop, each with its own mask save and restore.  In the first column the block above stands in for the missing left neighbour
// ((a + a + 1) >> 1 = a); 4 + p / 2 = (p + 8) >> 1 lies below p from 8 on and reaches 36 at the clamp.
__host__ __device__ __forceinline__ uint32_t HfNnzPredict(uint32_t bx, uint32_t by, uint32_t above, uint32_t left) {
  const uint32_t beside = bx == 0 ? above : left, edge = bx == 0 ? 32u : left, mean = (above + beside + 1) >> 1;
  const uint32_t top_row = by == 0 ? ~0u : 0u;
  return mean ^ ((mean ^ edge) & top_row);   // by == 0 ? edge : mean, kept a blend
}
__host__ __device__ __forceinline__ uint32_t HfNnzCountBucket(uint32_t predicted) {
  const uint32_t half = (predicted + 8) >> 1, lim = predicted < 36 ? predicted : 36;
  return half < lim ? half : lim;
}

// Integer sample of `bits` bits -> output sample (8 or 16 bits).  Equal depths pass through clamped; otherwise through a [0, 1]
// float, like the decoder library behind the reference does for every channel whose depth differs from the output type's.
__device__ __forceinline__ uint32_t IntToOutSample(int32_t v, int bits, int out_bits) {
  const int32_t maxv = (int32_t)((1u << bits) - 1);
  if (bits == out_bits) return (uint32_t)min(maxv, max(0, v));
  float f = (float)v * (1.0f / (float)maxv);
  f *= out_bits == 16 ? 65535.0f : 255.0f;
  const float top = out_bits == 16 ? 65535.0f : 255.0f;
  if (!(f > 0.f)) return 0;
  if (f >= top) return (uint32_t)top;
  return (uint32_t)(f + 0.5f);
}

// Bit pattern of a float-coded Modular sample (binary32 as is, binary16 widened) -> float
__device__ __forceinline__ float BitsToFloatSample(int32_t v, int bits) {
  if (bits == 32) return __int_as_float(v);
  return __half2float(__ushort_as_half((unsigned short)(v & 0xFFFF)));
}
__device__ __forceinline__ uint32_t FloatToOutBits(float f, int out_bits, int out_float) {
  if (out_float) return out_bits == 32 ? (uint32_t)__float_as_int(f) : (uint32_t)__half_as_ushort(__float2half_rn(f));
  const float top = out_bits == 16 ? 65535.0f : 255.0f;
  f *= top;
  if (!(f > 0.f)) return 0;
  if (f >= top) return (uint32_t)top;
  return (uint32_t)(f + 0.5f);
}
// One channel sample (integer of `bits` bits, or a float bit pattern when exp_bits > 0) -> raw bits of the output sample type
__device__ __forceinline__ uint32_t SampleToOutBits(int32_t v, int bits, int exp_bits, int out_bits, int out_float) {
  if (!out_float && !exp_bits) return IntToOutSample(v, bits, out_bits);
  const float f = exp_bits ? BitsToFloatSample(v, bits) : (float)v * (1.0f / (float)((1u << bits) - 1));
  return FloatToOutBits(f, out_bits, out_float);
}
__device__ __forceinline__ void StoreOutSample(uint8_t* base, size_t index, uint32_t raw, int out_bits) {
  if (out_bits == 8) base[index] = (uint8_t)raw;
  else if (out_bits == 16) ((uint16_t*)base)[index] = (uint16_t)raw;
  else ((uint32_t*)base)[index] = raw;
}

}  // namespace jxlhip
