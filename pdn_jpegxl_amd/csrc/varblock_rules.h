// The rules of a varblock, each stated once for host and device: which strategies exist and what each covers, orders and
// dequantises with; how a cell's 32-bit info word is packed; where coefficient (ky, kx) of a block lies in its stored form (the form
// of the coefficient orders and the dequantisation tables); where the basis of one transform length starts in the basis tables; which
// channel each of the three teams of a Y, X, B walk owns; and the dequantisation bias.  No kernel, no memory access beyond the
// constant tables below.  The decoder's placement and reconstruction (entropy_kernels.hip, kernels.hip, tile_kernels.hip), the
// encoder's front end (encode_kernels.hip, distance_kernels.hip), the host (host_parse.cc, batch_layout.cc) and the self tests all
// call these; the CPU suite holds every function against a statement written out in Python (tests/test_varblock_rules.py, through
// jxlhip_selftest_varblock_*).  Not here: the block-descriptor word of the HF decoder (HfUnpackBlock, entropy_kernels.hip) and the
// encoder's strategy byte (s | 0x80 on origins), which belong to their one producer and consumer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_types.h"

namespace jxlhip {

#define JXL_RULE __host__ __device__ __forceinline__

// ------------------------------------------------------------------ strategies
// By strategy id (DCT8, IDENTITY, DCT2X2, DCT4X4, DCT16X16, DCT32X32, DCT16X8, DCT8X16, DCT32X8, DCT8X32, DCT32X16, DCT16X32, DCT4X8,
// DCT8X4, AFV0..3, DCT64X64, DCT64X32, DCT32X64, DCT128X128, DCT128X64, DCT64X128, DCT256X256, DCT256X128, DCT128X256; the names
// give rows x columns): log2 of the cells covered across and down, the coefficient-order bucket and the dequantisation table.  Shapes
// that are transposes of each other share a bucket and a table.
constexpr uint8_t kStrategyLog2Cx[kNumStrategies] = {0, 0, 0, 0, 1, 2, 0, 1, 0, 2, 1, 2, 0, 0, 0, 0, 0, 0, 3, 2, 3, 4, 3, 4, 5, 4, 5};
constexpr uint8_t kStrategyLog2Cy[kNumStrategies] = {0, 0, 0, 0, 1, 2, 1, 0, 2, 0, 2, 1, 0, 0, 0, 0, 0, 0, 3, 3, 2, 4, 4, 3, 5, 5, 4};
constexpr uint8_t kStrategyOrderBucket[kNumStrategies] = {0, 1, 1, 1, 2, 3, 4, 4, 5, 5, 6, 6, 1, 1, 1, 1, 1, 1, 7, 8, 8, 9, 10, 10, 11, 12, 12};
constexpr uint8_t kStrategyQuantTable[kNumStrategies] = {0, 1, 2, 3, 4, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 10, 10, 11, 12, 12, 13, 14, 14, 15, 16, 16};

JXL_RULE bool StrategyValid(int s) { return s >= 0 && s < kNumStrategies; }
// (the four below index the tables: s is a valid id)
JXL_RULE int StrategyLog2Cx(uint32_t s) { return kStrategyLog2Cx[s]; }   // covered cells across = 1 << this
JXL_RULE int StrategyLog2Cy(uint32_t s) { return kStrategyLog2Cy[s]; }   // ... and down
JXL_RULE uint32_t StrategyOrderBucket(uint32_t s) { return kStrategyOrderBucket[s]; }
JXL_RULE uint32_t StrategyQuantTable(uint32_t s) { return kStrategyQuantTable[s]; }
// The 8x8 transforms that are no plain DCT (IDENTITY, DCT2X2, DCT4X4; DCT4X8, DCT8X4, AFV0..3): stored untransposed, reconstructed by
// idct_special_kernel.  The AFV ids are refused by the decoder (kErrUnsupportedTransform).
JXL_RULE bool StrategyIsSpecial(uint32_t s) { return (s >= 1 && s <= 3) || (s >= 12 && s <= 17); }
JXL_RULE bool StrategyIsAfv(uint32_t s) { return s >= 14 && s <= 17; }

// ------------------------------------------------------------------ the cell info word (DevImage::cellinfo)
// Per 8x8 cell: strategy | ix << 8 | iy << 13 | log2cx << 18 | log2cy << 21 | valid << 31, (ix, iy) the cell's place inside its
// varblock.  A word of zeros is a cell that no varblock was placed on.
constexpr uint32_t kCellValidBit = 1u << 31;
constexpr uint32_t kCellOffsetBits = 31u << 8 | 31u << 13;   // ix and iy
static_assert((kCellValidBit | kCellOffsetBits) == 0x8003FF00u, "valid, ix and iy are what an origin cell is told by");
JXL_RULE uint32_t CellInfoPack(uint32_t s, uint32_t ix, uint32_t iy, uint32_t lcx, uint32_t lcy) {
  return s | ix << 8 | iy << 13 | lcx << 18 | lcy << 21 | kCellValidBit;
}
JXL_RULE uint32_t CellStrategy(uint32_t info) { return info & 0xFF; }
JXL_RULE uint32_t CellIx(uint32_t info) { return (info >> 8) & 31; }
JXL_RULE uint32_t CellIy(uint32_t info) { return (info >> 13) & 31; }
JXL_RULE uint32_t CellLog2Cx(uint32_t info) { return (info >> 18) & 7; }
JXL_RULE uint32_t CellLog2Cy(uint32_t info) { return (info >> 21) & 7; }
JXL_RULE bool CellValid(uint32_t info) { return info >> 31; }
JXL_RULE bool CellIsOrigin(uint32_t info) { return (info & (kCellValidBit | kCellOffsetBits)) == kCellValidBit; }   // valid, ix = iy = 0

// ------------------------------------------------------------------ stored layout
// The coefficients of a varblock of 8 << lcy rows and 8 << lcx columns are stored with the longer side along a row: pitch
// 8 << max(lcx, lcy), (ky, kx) swapped when the block is at least as tall as wide (squares too); the special 8x8 transforms never
// swap.  The lowest (1 << lcy) x (1 << lcx) coefficients (LLF) come from the LF image, not from the HF stream.
JXL_RULE uint32_t StoredLog2Pitch(uint32_t lcx, uint32_t lcy) { return 3 + (lcx > lcy ? lcx : lcy); }
JXL_RULE bool StoredTransposed(bool special, uint32_t lcx, uint32_t lcy) { return !special && lcy >= lcx; }
JXL_RULE uint32_t StoredIndex(uint32_t ky, uint32_t kx, uint32_t log2_pitch, bool transposed) {
  return transposed ? (kx << log2_pitch) + ky : (ky << log2_pitch) + kx;
}
JXL_RULE void StoredToKyKx(uint32_t p, uint32_t log2_pitch, bool transposed, uint32_t* ky, uint32_t* kx) {
  const uint32_t r = p >> log2_pitch, c = p & ((1u << log2_pitch) - 1);
  *ky = transposed ? c : r;
  *kx = transposed ? r : c;
}
JXL_RULE bool IsLlfPosition(uint32_t ky, uint32_t kx, uint32_t lcx, uint32_t lcy) { return ky < (1u << lcy) && kx < (1u << lcx); }

// ------------------------------------------------------------------ basis tables
// basis_all holds the scaled N x N IDCT bases B[k * N + n] of N = 8, 16, ..., 256 back to back, basis_small the c x c ones of
// c = 1, 2, 4, ..., 32 (LLF from LF): where one starts.
JXL_RULE int BasisAllOffset(int N) { return (N * N - 64) / 3; }
JXL_RULE int BasisSmallOffset(int c) { return (c * c - 1) / 3; }

// ------------------------------------------------------------------ team order
// Walks over the three channels go Y, X, B (Y first: chroma from luma needs it): the channel of walk position i.
JXL_RULE int ChannelOfTeam(int i) { return i == 0 ? 1 : (i == 1 ? 0 : 2); }

// ------------------------------------------------------------------ dequantisation bias
// A quantised HF value v stands for 0, +-qb (the channel's bias) or v - qb3 / v.  `quotient(qb3, f)` says how qb3 / f is formed: the
// generic kernels and the encoder divide (ExactQuotient), recon_tile_kernel multiplies by the hardware reciprocal.
struct ExactQuotient {
  JXL_RULE float operator()(float a, float f) const { return a / f; }
};
template <class Quotient>
JXL_RULE float DequantBias(int32_t v, float qb, float qb3, Quotient quotient) {
  if (v == 0) return 0.f;
  if (v == 1) return qb;
  if (v == -1) return -qb;
  const float f = (float)v;
  return f - quotient(qb3, f);
}

#undef JXL_RULE

}  // namespace jxlhip
