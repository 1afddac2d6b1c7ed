// LDS-tiled and register-streaming pixel stages (gfx950).
//
//   recon_tile_kernel     one workgroup per 64x64 tile, all three channels: the sparse entry lists hf_decode_kernel wrote (one 32-bit
//                         entry per non-zero coefficient) are dequantised and scattered into three zeroed LDS tiles, chroma from
//                         luma added from the same luma entries, LF -> LLF, both IDCT passes in place (16x16 sub-blocks of varblocks
//                         >= 16 points on v_mfma_f32_16x16x4_f32), f32 XYB out (12 B/px).  Tiles that hold part of a varblock larger
//                         than the tile, a special 8x8 transform or a progressive frame go to a per-image list for the generic
//                         (unfused, any-size) kernels of kernels.hip.
//   filter_stream_kernel, filter_stream2_kernel
//                         Gaborish + EPF iteration 1 (+ colour and output, or f32 rows for) iteration 2 + colour and output: register
//                         streaming with DPP wave shifts, four pixels per lane, any width and output layout.
//   filter_stream_pairs_kernel, filter_stream2_pairs_kernel
//                         the same for frames of even width with 8-bit output (RGBA, RGB, gray + alpha, gray): two pixels per lane,
//                         buffer addressing, no load in a branch, four / eight wavefronts per SIMD.
//   filter_tile_kernel    one Gaborish / EPF stage on a 64x32 tile + halo staged in LDS (mirrored at the frame edge); the LAST
//                         enabled stage of an image converts XYB -> output samples and merges alpha.  Used for frames without EPF
//                         (Gaborish alone), for Gaborish and iteration 0 of three-iteration frames, and for the stage taps.
//   lf_output_kernel      reduced-size decode (1:8): the LF planes through the same pixel writers, one pixel per 8x8 cell; none of
//                         the kernels above runs for such a batch.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "dev_types.h"
#include "dev_util.h"
#include "kernels.h"
#include "lds_layout.h"
#include "varblock_rules.h"

namespace jxlhip {

// Wavefront issue priority of the pixel kernels, for tools/ab_prio.sh.  Measured in the pipelined step (round 3): 1 or 3 make
// the streaming filters slower (filters + output 51 -> 82 ms per batch, step 123 -> 148 ms), so the default emits no instruction.
#ifndef JXLHIP_PRIO_PIXEL
#define JXLHIP_PRIO_PIXEL 0
#endif
#if JXLHIP_PRIO_PIXEL
#define JXL_PIXEL_PRIO() __builtin_amdgcn_s_setprio(JXLHIP_PRIO_PIXEL)
#else
#define JXL_PIXEL_PRIO() ((void)0)
#endif

namespace {

constexpr int kTS = kReconTileSide;    // tile side
constexpr int kLP = kReconTilePitch;   // LDS pitch (conflict-free column walks)

typedef float __attribute__((ext_vector_type(4))) F4;
// a 16x16 sub-block (2x2 cells at even cell coordinates) goes to the matrix cores, per pass, when the varblocks of its cells are at
// least 16 points long in the pass's direction, of one length and at one offset (MfmaRows / MfmaCols below)
// One 16x16 output sub-block: acc = sum_k A[k] * B[k] with both operand streams fetched up front (N / 4 independent loads
// each, one wait) so that the MFMA chain is not paced by a memory round trip per step.  pa / pb: lane's first operand;
// sa / sb: stride between consecutive k-steps of four.
template <int N>
__device__ __forceinline__ F4 MfmaChain(const float* pa, int sa, const float* pb, int sb) {
  float a[N / 4], b[N / 4];
#pragma unroll
  for (int k = 0; k < N / 4; k++) { a[k] = pa[k * sa]; b[k] = pb[k * sb]; }
  F4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < N / 4; k++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[k], b[k], acc, 0, 0, 0);
  return acc;
}
// 32- and 64-point passes: one operand stream is the k-contiguous basis table (basis_mfma: for a lane (n, q) the N / 4 values
// basis[(4 k + q) * N + n], k = 0 .. N/4-1, lie side by side), read from an LDS copy (arrays of 16-byte pieces, so that consecutive
// (n, q) lanes read consecutive 16 bytes): from global memory every 16x16 sub-block paid two to four dependent L2 round trips before
// its first MFMA.
template <bool kTableIsA>
__device__ __forceinline__ F4 MfmaChain32L(const float4* t_lo, const float4* t_hi, int pair, const float* po, int so) {
  const float4 v0 = t_lo[pair], v1 = t_hi[pair];
  const float t[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
  float o[8];
#pragma unroll
  for (int k = 0; k < 8; k++) o[k] = po[k * so];
  F4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 8; k++)
    acc = kTableIsA ? __builtin_amdgcn_mfma_f32_16x16x4f32(t[k], o[k], acc, 0, 0, 0) : __builtin_amdgcn_mfma_f32_16x16x4f32(o[k], t[k], acc, 0, 0, 0);
  return acc;
}
// The 64-point table likewise (four arrays of 16-byte quarters; staged only by tiles that hold a 64-point varblock): from global
// memory a sub-block paid four dependent L2 round trips before its sixteen MFMAs, and a fifth of this content's area is 64 points long.
template <bool kTableIsA>
__device__ __forceinline__ F4 MfmaChain64L(const float4* t64, int pair, const float* po, int so) {
  float t[16], o[16];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const float4 v = t64[j * 256 + pair];
    t[4 * j] = v.x; t[4 * j + 1] = v.y; t[4 * j + 2] = v.z; t[4 * j + 3] = v.w;
  }
#pragma unroll
  for (int k = 0; k < 16; k++) o[k] = po[k * so];
  F4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 16; k++)
    acc = kTableIsA ? __builtin_amdgcn_mfma_f32_16x16x4f32(t[k], o[k], acc, 0, 0, 0) : __builtin_amdgcn_mfma_f32_16x16x4f32(o[k], t[k], acc, 0, 0, 0);
  return acc;
}
// Per pass, a 16x16 sub-block only needs ONE transform length and phase over its 16 columns (vertical pass) or rows (horizontal pass):
// the two cells across the pass direction must belong to varblocks of the same length in that direction, at the same offset - they
// need not be the same varblock (16x8 blocks side by side, a 32x16 beside a 32x32 ...).  With the one-varblock test alone, every
// rectangular block of 8 points in the other direction fell back to the vector-ALU loops (a fifth of this content's cells).
__device__ __forceinline__ bool MfmaRows(uint32_t tl, uint32_t tr) {   // vertical pass: rows >= 16, same length and row offset
  const uint32_t ll = CellLog2Cy(tl), lr = CellLog2Cy(tr), ol = CellIy(tl), orr = CellIy(tr);
  return CellValid(tl) && CellValid(tr) && ll >= 1 && ll == lr && ol == orr;
}
__device__ __forceinline__ bool MfmaCols(uint32_t tl, uint32_t bl) {   // horizontal pass: columns >= 16, same length and column offset
  const uint32_t lt = CellLog2Cx(tl), lb = CellLog2Cx(bl), ot = CellIx(tl), ob = CellIx(bl);
  return CellValid(tl) && CellValid(bl) && lt >= 1 && lt == lb && ot == ob;
}

// v^(1/2.4) through the hardware log2 / exp2 (v_log_f32, v_exp_f32: about 1 ulp each, i.e. < 1e-3 of an 8-bit step after the
// * 255) instead of the ~50-instruction powf: the colour conversion was 46 % of the fused filter kernel.
__device__ __forceinline__ float SrgbOetfT(float v) {
  // both branches are computed and selected (v_cndmask): as a conditional the compiler emitted an exec-mask branch per sample
  const float lin = 12.92f * v;
  const float cur = 1.055f * __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(v) * (1.0f / 2.4f)) - 0.055f;
  return v <= 0.0031308f ? lin : cur;
}
// the same curve scaled to 0 .. 255 (the 8-bit output path)
__device__ __forceinline__ float SrgbOetf255T(float v) {
  const float lin = (12.92f * 255.0f) * v;
  const float cur = (1.055f * 255.0f) * __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(v) * (1.0f / 2.4f)) - (0.055f * 255.0f);
  return v <= 0.0031308f ? lin : cur;
}
__device__ __forceinline__ float PowT(float a, float e) { return __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(a) * e); }   // a > 0
// Encoded value from display-linear, sign-symmetric like the reference's library.  kind: 0 linear, 1 sRGB, 2 BT.709, 3 PQ,
// 5 table (4096 entries over sqrt(linear), clamped to [0, 1]: an evaluated ICC tone curve).
__device__ __forceinline__ float EncodeTransferT(int kind, float v, float pq_scale, const float* lut = nullptr) {
  if (kind == 0) return v;
  if (kind == 5) {
    const float t = __builtin_sqrtf(fminf(fmaxf(v, 0.f), 1.f)) * 4095.0f;
    const int i = min((int)t, 4094);
    return lut[i] + (lut[i + 1] - lut[i]) * (t - (float)i);
  }
  const float a = fabsf(v);
  float r;
  if (kind == 1) r = a <= 0.0031308f ? 12.92f * a : 1.055f * PowT(a, 1.0f / 2.4f) - 0.055f;
  else if (kind == 2) r = a < 0.018f ? 4.5f * a : 1.099f * PowT(a, 0.45f) - 0.099f;
  else {
    const float xp = a > 0.f ? PowT(a * pq_scale, 0.1593017578125f) : 0.f;
    r = a > 0.f ? PowT((0.8359375f + 18.8515625f * xp) / (1.0f + 18.6875f * xp), 78.84375f) : 0.f;
  }
  return copysignf(r, v);
}
__device__ __forceinline__ uint8_t ToU8T(float v) {   // round half up, clamped; NaN -> 0 (v_max_f32 returns the other operand)
  v = fminf(fmaxf(v * 255.0f, 0.f), 255.0f);
  return (uint8_t)(v + 0.5f);
}

// The alpha plane holds samples of the output type (alpha_finish_kernel scales them): one u8 or u16 load.
__device__ __forceinline__ uint32_t LoadAlpha(const DevImage& im, size_t i) {
  return im.out_bits == 8 ? (uint32_t)im.alpha[i] : (im.out_bits == 16 ? (uint32_t)((const uint16_t*)im.alpha)[i] : ((const uint32_t*)im.alpha)[i]);
}
// `a`: the pixel's alpha sample (ignored by layouts without alpha), fetched by the caller ahead of the arithmetic; `position()`: the
// pixel's index in the output buffer (the full-size writers address it by the frame's geometry, lf_output_kernel by the reduced
// one), evaluated after the arithmetic
template <typename Position>
__device__ __forceinline__ void WritePixelAt(const DevImage& im, Position position, float X, float Y, float B, uint32_t a) {
  const float gr = Y + X - im.opsin_bias_cbrt[0], gg = Y - X - im.opsin_bias_cbrt[1], gb = B - im.opsin_bias_cbrt[2];
  const float mr = gr * gr * gr + im.opsin_bias[0], mg = gg * gg * gg + im.opsin_bias[1], mb = gb * gb * gb + im.opsin_bias[2];
  float r = im.opsin_inv[0] * mr + im.opsin_inv[1] * mg + im.opsin_inv[2] * mb;
  float g = im.opsin_inv[3] * mr + im.opsin_inv[4] * mg + im.opsin_inv[5] * mb;
  float bl = im.opsin_inv[6] * mr + im.opsin_inv[7] * mg + im.opsin_inv[8] * mb;
  if (im.to_srgb == 1 && !im.out_float) {
    // the common case on its own short path (integer outputs clamp negatives to 0 anyway, so the curve need not be sign-symmetric here)
    r = SrgbOetfT(r); g = SrgbOetfT(g); bl = SrgbOetfT(bl);
  } else if (im.to_srgb) {
    r = EncodeTransferT(im.to_srgb, r, im.pq_scale, im.trc_lut); g = EncodeTransferT(im.to_srgb, g, im.pq_scale, im.trc_lut + 4096);
    bl = EncodeTransferT(im.to_srgb, bl, im.pq_scale, im.trc_lut + 8192);
  }
  if (im.unpremultiply) {   // associated alpha: the encoded samples are divided by max(alpha, 2^-26) (Decoder/JxlDecoder.cpp:233)
    const float m = 1.0f / fmaxf(1.0f / 67108864.0f, (float)a * im.alpha_unit);
    r *= m; g *= m; bl *= m;
  }
  const size_t o = position();
  if (im.out_bits != 8) {   // u16 above 8 bits per sample, f16 / f32 for float samples (Decoder/JxlDecoder.cpp:510-548); `a` is raw bits
    const size_t b = o * im.nch_out;
    if (im.ncolor == 3) {
      StoreOutSample(im.out, b, FloatToOutBits(r, im.out_bits, im.out_float), im.out_bits);
      StoreOutSample(im.out, b + 1, FloatToOutBits(g, im.out_bits, im.out_float), im.out_bits);
      StoreOutSample(im.out, b + 2, FloatToOutBits(bl, im.out_bits, im.out_float), im.out_bits);
      if (im.has_alpha) StoreOutSample(im.out, b + 3, a, im.out_bits);
    } else {
      StoreOutSample(im.out, b, FloatToOutBits(g, im.out_bits, im.out_float), im.out_bits);
      if (im.has_alpha) StoreOutSample(im.out, b + 1, a, im.out_bits);
    }
    return;
  }
  if (im.nch_out == 4) {
    uchar4 px;
    px.x = ToU8T(r); px.y = ToU8T(g); px.z = ToU8T(bl); px.w = (uint8_t)a;
    ((uchar4*)im.out)[o] = px;
  } else {
    uint8_t* out = im.out + o * im.nch_out;
    if (im.ncolor == 3) {
      out[0] = ToU8T(r); out[1] = ToU8T(g); out[2] = ToU8T(bl);
    } else {
      out[0] = ToU8T(g);
      if (im.has_alpha) out[1] = (uint8_t)a;
    }
  }
}
__device__ __forceinline__ void WritePixelA(const DevImage& im, int x, int y, float X, float Y, float B, uint32_t a) {
  WritePixelAt(im, [&] { return (size_t)(y - im.band_y0) * im.w + x; }, X, Y, B, a);   // position in the output band
}
// The common layouts (u8 samples, sRGB or linear transfer) without the branches of the general function: used by the fused filter
// kernel, whose output phase is a large part of its time.
// (frames with noise take the general path of the streaming kernels: the addition lives in WritePixelGeneral / WritePixel only)
__device__ __forceinline__ bool PlainOutput(const DevImage& im) { return im.out_bits == 8 && im.to_srgb <= 1 && !im.unpremultiply && !im.has_noise; }
// Synthetic noise (rule 4): the strength for intensity v from the frame's eight-entry table, linear between entries
__device__ __forceinline__ float NoiseStrength(const DevImage& im, float v) {
  const float s = fmaxf(0.f, 6.0f * v);
  const int i = (int)fminf(s, 6.0f);
  const float t = fminf(s - (float)i, 1.0f);
  const float lo = im.noise_lut[i], hi = im.noise_lut[i + 1];
  return fminf(fmaxf(lo + (hi - lo) * t, 0.f), 1.0f);
}
// ... and the addition of the convolved planes (noise_kernels.hip) to a filtered XYB pixel, before the inverse opsin transform
__device__ __forceinline__ void AddNoise(const DevImage& im, int x, int y, float& X, float& Y, float& B) {
  const size_t o = (size_t)y * im.w + x;
  const float n0 = im.noise[0][o], n1 = im.noise[1][o], n2 = im.noise[2][o];
  const float sr = NoiseStrength(im, 0.5f * (Y + X)), sg = NoiseStrength(im, 0.5f * (Y - X));
  const float shared = n2 * (127.0f / 128.0f);
  const float red = (n0 * (1.0f / 128.0f) + shared) * sr, green = (n1 * (1.0f / 128.0f) + shared) * sg;
  const float rg = red + green;
  X += im.base_x * rg + (red - green);
  Y += rg;
  B += im.base_b * rg;
}
// XYB -> sRGB-encoded u8 (the plain output layouts)
__device__ __forceinline__ uint32_t PixelToRgba8(const DevImage& im, float X, float Y, float B, uint32_t a) {
  const float gr = Y + X - im.opsin_bias_cbrt[0], gg = Y - X - im.opsin_bias_cbrt[1], gb = B - im.opsin_bias_cbrt[2];
  const float mr = gr * gr * gr + im.opsin_bias[0], mg = gg * gg * gg + im.opsin_bias[1], mb = gb * gb * gb + im.opsin_bias[2];
  float r = im.opsin_inv[0] * mr + im.opsin_inv[1] * mg + im.opsin_inv[2] * mb;
  float g = im.opsin_inv[3] * mr + im.opsin_inv[4] * mg + im.opsin_inv[5] * mb;
  float bl = im.opsin_inv[6] * mr + im.opsin_inv[7] * mg + im.opsin_inv[8] * mb;
  // to 8 bits with v_cvt_pk_u8_f32: converts (round to nearest, ties to even - tools/cvt_probe.hip), saturates to 0 .. 255, maps NaN to
  // 0 and inserts the byte, in ONE instruction per channel instead of scale / max / min / add / convert / shift / or; the * 255 is
  // folded into the transfer curve's constants.  (Differs from round-half-up only on exact ties.)
  if (im.to_srgb) { r = SrgbOetf255T(r); g = SrgbOetf255T(g); bl = SrgbOetf255T(bl); }
  else { r *= 255.0f; g *= 255.0f; bl *= 255.0f; }
  uint32_t px = a << 24;
  px = __builtin_amdgcn_cvt_pk_u8_f32(r, 0, px);
  px = __builtin_amdgcn_cvt_pk_u8_f32(g, 1, px);
  px = __builtin_amdgcn_cvt_pk_u8_f32(bl, 2, px);
  return px;
}
// Out of line on purpose: inlined four times into the fused filter kernel's unrolled output phase, the general function more than
// doubled that kernel's code (2.3 k -> 5.8 k instructions) and cost 8 % of its speed on the plain path that never executes it.
__device__ __noinline__ void WritePixelGeneral(const DevImage& im, int x, int y, float X, float Y, float B, uint32_t a) {
  if (im.has_noise) {
    AddNoise(im, x, y, X, Y, B);
    // 8-bit sRGB / linear layouts: the conversion this pixel gets in the same frame without noise (PixelToRgba8 in the pair kernels
    // and for the whole RGBA quads of the four-pixel kernels, WritePixelA elsewhere), so that noise of strength zero changes no byte
    if (im.out_bits == 8 && im.to_srgb <= 1 && !im.unpremultiply && im.final_stage == 5 &&
        (im.noise_pairs_twin || (im.nch_out == 4 && (x | 3) < im.w))) {
      const uint32_t px = PixelToRgba8(im, X, Y, B, a);
      uint8_t* out = im.out + ((size_t)(y - im.band_y0) * im.w + x) * im.nch_out;
      if (im.nch_out == 4) *(uint32_t*)out = px;
      else if (im.nch_out == 3) { out[0] = (uint8_t)px; out[1] = (uint8_t)(px >> 8); out[2] = (uint8_t)(px >> 16); }
      else { out[0] = (uint8_t)(px >> 8); if (im.nch_out == 2) out[1] = (uint8_t)(px >> 24); }
      return;
    }
  }
  WritePixelA(im, x, y, X, Y, B, a);
}
__device__ __forceinline__ void WritePixel(const DevImage& im, int x, int y, float X, float Y, float B) {
  const uint32_t a = im.has_alpha ? LoadAlpha(im, (size_t)y * im.w + x) : 0u;
  if (im.has_noise) { WritePixelGeneral(im, x, y, X, Y, B, a); return; }   // (out of line: the stage kernels keep their registers)
  WritePixelA(im, x, y, X, Y, B, a);
}

}  // namespace

// ------------------------------------------------------------------ fused reconstruction of one 64x64 tile
// one basis row (8 outputs) times two inputs: every basis fetch feeds 16 FMAs
#define JXL_IDCT_STEP(Bp, v0, v1)                                                                  \
  {                                                                                                \
    const float4 b0 = *(const float4*)(Bp);                                                        \
    const float4 b1 = *(const float4*)((Bp) + 4);                                                  \
    a0[0] += v0 * b0.x; a0[1] += v0 * b0.y; a0[2] += v0 * b0.z; a0[3] += v0 * b0.w;                \
    a0[4] += v0 * b1.x; a0[5] += v0 * b1.y; a0[6] += v0 * b1.z; a0[7] += v0 * b1.w;                \
    a1[0] += v1 * b0.x; a1[1] += v1 * b0.y; a1[2] += v1 * b0.z; a1[3] += v1 * b0.w;                \
    a1[4] += v1 * b1.x; a1[5] += v1 * b1.y; a1[6] += v1 * b1.z; a1[7] += v1 * b1.w;                \
  }

constexpr int kTileF = kReconTileFloats;   // floats of one channel's tile

// The workgroup's LDS, carved as ReconTileLds (lds_layout.h) describes it; the fields are named and explained there.  Every phase makes
// its own view (the addresses are constants).
extern __shared__ __align__(16) uint8_t recon_lds[];
// Who a thread is among the workgroup's 12 wavefronts: team = wave / 4 owns channel Y, X, B, tw is the wavefront's place in its team.
// (Every phase derives it from threadIdx itself, so that the compiler sees the ranges there.)
struct ReconLane {
  int tid, lane, team, tw;
  __device__ __forceinline__ ReconLane() : tid(threadIdx.x), lane(tid & 63), team(tid >> 8), tw((tid >> 6) & 3) {}
};
struct ReconTile {
  float *cfc3, *B816, *cscale;
  uint32_t *ci, *cmeta, *cnq, *cpre, *cstart, *ctot;
  const U32x2** csc;
  float4 *t32_lo, *t32_hi, *t64;
  __device__ __forceinline__ ReconTile() {
    constexpr ReconTileLds L;
    uint8_t* const smem = recon_lds;
    cfc3 = (float*)(smem + L.cfc3); B816 = (float*)(smem + L.B816); cscale = (float*)(smem + L.cscale);
    ci = (uint32_t*)(smem + L.ci); cmeta = (uint32_t*)(smem + L.cmeta); cnq = (uint32_t*)(smem + L.cnq);
    cpre = (uint32_t*)(smem + L.cpre); cstart = (uint32_t*)(smem + L.cstart); ctot = (uint32_t*)(smem + L.ctot);
    csc = (const U32x2**)(smem + L.csc);
    t32_lo = (float4*)(smem + L.t32_lo); t32_hi = (float4*)(smem + L.t32_hi); t64 = (float4*)(smem + L.t64);
  }
};

// Per-cell set-up, by wavefront 0 (lane = cell of the tile): owns ci, cscale, cmeta, cnq, csc, the entry-list prefixes cpre / cstart of
// the three teams and ctot.  Returns whether this lane's cell makes the tile one for the generic kernels.
__device__ __forceinline__ int ReconCellSetup(const DevImage& im, int tx, int ty) {
  const ReconTile T;
  const int tid = threadIdx.x;
  int bad = 0;
  const int cx = tx * 8 + (tid & 7), cy = ty * 8 + (tid >> 3);
  const bool inside = cx < im.w8 && cy < im.h8;
  const size_t cell_g = (size_t)min(cy, im.h8 - 1) * im.w8 + min(cx, im.w8 - 1);
  const size_t ncells = (size_t)im.w8 * im.h8;
  const uint32_t info_g = im.cellinfo[cell_g];
  const uint32_t rq_g = im.rawq[cell_g];
  U32x2 blk[3];
  blk[0] = im.cblk[ncells + cell_g]; blk[1] = im.cblk[cell_g]; blk[2] = im.cblk[2 * ncells + cell_g];   // team order: Y, X, B
  const uint32_t info = inside ? info_g : 0u;
  const uint32_t rqv = inside ? rq_g : 1u;
  const int ix = CellIx(info), iy = CellIy(info), lcx = CellLog2Cx(info), lcy = CellLog2Cy(info);
  if (inside) {
    if (!CellValid(info)) bad = 1;
    else {
      const int ox = (tid & 7) - ix, oy = (tid >> 3) - iy;
      // blocks larger than the tile, the rare special 8x8 transforms, and blocks that do not start on a multiple of their own size
      // (every encoder aligns them, the format's placement rule does not; the matrix-core sub-blocks below rely on it) are left
      // to the generic kernels
      bad = ox < 0 || oy < 0 || ox + (1 << lcx) > 8 || oy + (1 << lcy) > 8 || StrategyIsSpecial(CellStrategy(info)) ||
            (ox & ((1 << lcx) - 1)) != 0 || (oy & ((1 << lcy) - 1)) != 0;
    }
  }
  const bool valid = CellValid(info) && !bad;
  const int has64 = valid && (lcx == 3 || lcy == 3);
  {  // (wavefront 0 is the only writer of the per-cell tables; the flag travels with them through the barrier behind the set-up)
    const uint64_t any = __ballot(has64);
    if (tid == 0) T.ctot[3] = any != 0;
  }
  const uint32_t q = StrategyQuantTable(valid ? CellStrategy(info) : 0);
  const uint32_t rq_origin = (uint32_t)__shfl((int)rqv, valid ? tid - iy * 8 - ix : tid);
  T.ci[tid] = info;
  T.cscale[tid] = im.inv_global_scale / (float)rq_origin;
  T.cmeta[tid] = StoredLog2Pitch(lcx, lcy) | (StoredTransposed(false, lcx, lcy) ? 16u : 0u);   // (no special transform gets this far)
  T.cnq[tid] = im.dq_n[q];
  T.csc[tid] = im.scan[q];
  // entry lists of the varblocks that start in this tile; a list a failed section left unwritten is treated as empty
  const bool origin = valid && ix == 0 && iy == 0;
  uint32_t cnt[3], sum[3];
#pragma unroll
  for (int t = 0; t < 3; t++) {
    cnt[t] = origin ? blk[t].y : 0u;
    if (cnt[t] > 65536u || blk[t].x > kGroupEntriesCap - cnt[t]) cnt[t] = 0;
    sum[t] = cnt[t];   // inclusive scans over the wavefront
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
    for (int t = 0; t < 3; t++) {
      const uint32_t a = (uint32_t)__shfl_up((int)sum[t], d);
      if (tid >= d) sum[t] += a;
    }
  }
#pragma unroll
  for (int t = 0; t < 3; t++) {
    T.cpre[t * 64 + tid] = sum[t] - cnt[t];
    T.cstart[t * 64 + tid] = blk[t].x;
    if (tid == 63) T.ctot[t] = sum[t];
  }
  return bad;
}

// LLF, by the first wavefront of each team (lane = cell): the lowest cx * cy coefficients of every varblock are the scaled 2-D DCT of
// its LF samples, formed with lane shuffles and added into the team's tile `cfc` while the other wavefronts scatter.
__device__ __forceinline__ void ReconLlf(const DevImage& im, int tx, int ty, const float* basis_small, const float* llf_scale) {
  const ReconTile T;
  const ReconLane me;
  const int lane = me.lane, c = ChannelOfTeam(me.team);
  float* const cfc = T.cfc3 + me.team * kTileF;
  const int cxg = tx * 8 + (lane & 7), cyg = ty * 8 + (lane >> 3);
  const bool inside = cxg < im.w8 && cyg < im.h8;
  const float lf_g = im.lf_final[c][(size_t)min(cyg, im.h8 - 1) * im.w8 + min(cxg, im.w8 - 1)];
  const float lfv = inside ? lf_g : 0.f;
  const uint32_t info = T.ci[lane];
  const bool valid = CellValid(info);
  const int ix = CellIx(info), iy = CellIy(info), lcx = CellLog2Cx(info), lcy = CellLog2Cy(info);
  const int cx = 1 << lcx, cy = 1 << lcy;
  const int ox = (lane & 7) - ix, oy = (lane >> 3) - iy;
  const float* Bx = basis_small + BasisSmallOffset(cx) + ix * cx;
  const float* By = basis_small + BasisSmallOffset(cy) + iy * cy;
  float bx[8], byv[8];
#pragma unroll
  for (int k = 0; k < 8; k++) { bx[k] = (valid && k < cx) ? Bx[k] : 0.f; byv[k] = (valid && k < cy) ? By[k] : 0.f; }
  const float sc = valid ? llf_scale[lcy * 32 + iy] * llf_scale[lcx * 32 + ix] / (float)(cx * cy) : 0.f;
  float row = 0.f;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const float v = __shfl(lfv, (lane - ix + k) & 63);
    if (valid && k < cx) row += v * bx[k];
  }
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const float v = __shfl(row, ((oy + k) * 8 + (lane & 7)) & 63);
    if (valid && k < cy) acc += v * byv[k];
  }
  // (an add like the entries': a custom coefficient order may send an entry to an LLF position, and sums do not depend on who comes first)
  if (valid) atomicAdd(&cfc[(oy * 8 + iy) * kLP + ox * 8 + ix], acc * sc);
}

// 1 / v through v_rcp_f32 (1 ulp; the term is a bias correction <= 0.15 / |v|)
struct RcpQuotient {
  __device__ __forceinline__ float operator()(float a, float f) const { return a * __builtin_amdgcn_rcpf(f); }
};

// The entry scatter, by all 768 threads: every entry of the tile's (block, channel) lists is one non-zero quantised coefficient; its
// scan position k selects {stored index, weight} from the per-table scan list, the stored index gives the coefficient's place in the
// varblock.  The lists of the three channels are walked as ONE range [0, T_y + T_x + T_b) (a 4K frame has about 270 luma and 30 + 30
// chroma entries per tile: one trip).  An entry's cell comes from a binary search over the exclusive prefix of its channel's per-cell
// entry counts (only origin cells have entries).  A luma entry is also what chroma from luma adds to X and B - the IDCT is linear and
// the tile is inside one 64x64 chroma-from-luma tile - so it is added three times (dequantised once).  Adds into the zeroed tiles with
// ds_add_f32: a position receives at most one own addend and one luma addend, two addends commute, so the sums do not depend on the
// order the lanes arrive in.
__device__ __forceinline__ void ReconScatter(const DevImage& im, int tx, int ty) {
  const ReconTile T;
  const int tid = threadIdx.x;
  const size_t tile_cfl = (size_t)ty * im.wt + tx;
  const float cfl_x = im.base_x + (float)im.ytox[tile_cfl] * im.inv_color_factor;
  const float cfl_b = im.base_b + (float)im.ytob[tile_cfl] * im.inv_color_factor;
  // the tile's group (four tiles per group side)
  const uint32_t* entries = im.centries + (size_t)((ty >> 2) * im.xg + (tx >> 2) - im.centries_g0) * kGroupEntriesCap;
  const uint32_t t0 = T.ctot[0], t01 = t0 + T.ctot[1], total = t01 + T.ctot[2];
  const float qb3 = im.qbias[3];
  for (uint32_t e = (uint32_t)tid; e < total; e += 768) {
    const uint32_t t = (e >= t0) + (e >= t01);                     // team of this entry: 0 Y, 1 X, 2 B
    const uint32_t el = e - (t == 0 ? 0u : (t == 1 ? t0 : t01));
    const uint32_t* pre = T.cpre + t * 64;
    uint32_t j = 0;
#pragma unroll
    for (int step = 32; step; step >>= 1) if (pre[j + step] <= el) j += step;
    const uint32_t ent = entries[T.cstart[t * 64 + j] + (el - pre[j])];
    const uint32_t k = ent & 0xFFFFu, nq = T.cnq[j];
    if (k >= nq) continue;   // a list that a failed section left half-written must not index past the table
    const int chan = ChannelOfTeam(t);
    const U32x2 se = T.csc[j][(size_t)chan * nq + k];
    const uint32_t meta = T.cmeta[j];
    uint32_t ky, kx;
    StoredToKyKx(se.x, meta & 15, meta & 16, &ky, &kx);
    if (ky >= 64 || kx >= 64) continue;
    const int32_t v = (int32_t)ent >> 16;
    const float dm = t == 0 ? 1.0f : (t == 1 ? im.x_dm : im.b_dm);
    const float o = DequantBias(v, im.qbias[chan], qb3, RcpQuotient()) * (T.cscale[j] * dm) * __uint_as_float(se.y);
    const uint32_t at = ((j >> 3) * 8 + ky) * kLP + (j & 7) * 8 + kx;
    atomicAdd(&T.cfc3[t * kTileF + at], o);
    if (t == 0) {   // chroma from luma: X += cfl_x * Y, B += cfl_b * Y on the dequantised luma coefficient
      if (cfl_x != 0.f) atomicAdd(&T.cfc3[kTileF + at], o * cfl_x);
      if (cfl_b != 0.f) atomicAdd(&T.cfc3[2 * kTileF + at], o * cfl_b);
    }
  }
}

// The two 1-D IDCT passes over a team's tile, in place, each of the team's four wavefronts on its own share: the vertical pass gives
// wavefront tw the column stripe [16 tw, 16 tw + 16) (everything a stripe's outputs depend on lies in the same columns), the
// horizontal pass the row band [16 tw, 16 tw + 16).  A wavefront fetches all its operands before it stores, so a pass needs no
// workgroup barrier inside.  The matrix cores take every 16x16 sub-block whose two cells across the pass agree (MfmaRows / MfmaCols):
// vertical Basis_R^T (16 x R) * coefficients (R x 16), horizontal rows (16 x C) * Basis_C (C x 16), by v_mfma_f32_16x16x4_f32 (exact
// f32, the same k-ordered fma chain as the vector path).  Lane l feeds A[l & 15][l >> 4] and B[l >> 4][l & 15], owns
// D[4 * (l >> 4) + r][l & 15].  The vector ALUs take the rest: one lane = two adjacent lines x one 8-sample cell.
// (Mirror images kept as two functions: merged into one template the kernel compiled to 8 - 10 % more instructions and two more VGPRs.)
__device__ __forceinline__ void ReconVerticalPass(const float* Bl) {
  const ReconTile T;
  const ReconLane me;
  const int lane = me.lane, tw = me.tw;
  float* const cfc = T.cfc3 + me.team * kTileF;   // this team's tile
  const uint32_t* ci = T.ci;
  float* B816 = T.B816;
  const int l16 = lane & 15, lq = lane >> 4;
  F4 acc[4];
  bool m[4];
  const int x0 = tw * 16;
#pragma unroll
  for (int rb = 0; rb < 4; rb++) {
    const uint32_t inf = ci[rb * 16 + tw * 2];
    m[rb] = MfmaRows(inf, ci[rb * 16 + tw * 2 + 1]);   // wave-uniform
    if (m[rb]) {
      const int iy = CellIy(inf), lcy = CellLog2Cy(inf), R = 8 << lcy;
      const float* cp = cfc + ((rb * 2 - iy) * 8 + lq) * kLP + x0 + l16;
      if (R == 16) acc[rb] = MfmaChain<16>(B816 + 64 + lq * 16 + iy * 8 + l16, 64, cp, 4 * kLP);
      else if (R == 32) acc[rb] = MfmaChain32L<true>(T.t32_lo, T.t32_hi, (iy * 8 + l16) * 4 + lq, cp, 4 * kLP);
      else acc[rb] = MfmaChain64L<true>(T.t64, (iy * 8 + l16) * 4 + lq, cp, 4 * kLP);
    }
  }
  // the rest on the vector ALUs.  One lane = two adjacent columns x one 8-row cell: every basis fetch feeds 16 FMAs.
  const int x = x0 + (lane & 7) * 2, cr = lane >> 3;
  const uint32_t info = ci[cr * 8 + (x >> 3)];
  const bool valu = CellValid(info) && !MfmaRows(ci[(cr >> 1) * 16 + (x >> 4) * 2], ci[(cr >> 1) * 16 + (x >> 4) * 2 + 1]);
  float a0[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (valu) {
    const int iy = CellIy(info), lcy = CellLog2Cy(info);
    const int R = 8 << lcy;
    const float* in = cfc + (cr - iy) * 8 * kLP + x;
    if (R == 8) {            // the common sizes read their basis from LDS: no global load inside the pass
#pragma unroll 2
      for (int k = 0; k < 8; k++) { const float v0 = in[k * kLP], v1 = in[k * kLP + 1]; JXL_IDCT_STEP(B816 + k * 8, v0, v1) }
    } else if (R == 16) {
      const float* B = B816 + 64 + iy * 8;
#pragma unroll 2
      for (int k = 0; k < 16; k++) { const float v0 = in[k * kLP], v1 = in[k * kLP + 1]; JXL_IDCT_STEP(B + k * 16, v0, v1) }
    } else {
      const float* B = Bl + BasisAllOffset(R) + iy * 8;
      for (int k = 0; k < R; k++) { const float v0 = in[k * kLP], v1 = in[k * kLP + 1]; JXL_IDCT_STEP(B + k * R, v0, v1) }
    }
  }
  // every operand of this stripe is in registers: store
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int rb = 0; rb < 4; rb++)
    if (m[rb]) {
      float* o = cfc + (rb * 16 + 4 * lq) * kLP + x0 + l16;
      o[0] = acc[rb].x; o[kLP] = acc[rb].y; o[2 * kLP] = acc[rb].z; o[3 * kLP] = acc[rb].w;
    }
  if (valu) {
#pragma unroll
    for (int j = 0; j < 8; j++) { cfc[(cr * 8 + j) * kLP + x] = a0[j]; cfc[(cr * 8 + j) * kLP + x + 1] = a1[j]; }
  }
}

__device__ __forceinline__ void ReconHorizontalPass(const float* Bl) {
  const ReconTile T;
  const ReconLane me;
  const int lane = me.lane, tw = me.tw;
  float* const cfc = T.cfc3 + me.team * kTileF;   // this team's tile
  const uint32_t* ci = T.ci;
  float* B816 = T.B816;
  const int l16 = lane & 15, lq = lane >> 4;
  F4 acc[4];
  bool m[4];
  const int y0 = tw * 16;
#pragma unroll
  for (int cs = 0; cs < 4; cs++) {
    const uint32_t inf = ci[tw * 16 + cs * 2];
    m[cs] = MfmaCols(inf, ci[tw * 16 + 8 + cs * 2]);
    if (m[cs]) {
      const int ix = CellIx(inf), lcx = CellLog2Cx(inf), C = 8 << lcx;
      const float* ap = cfc + (y0 + l16) * kLP + (cs * 2 - ix) * 8 + lq;
      if (C == 16) acc[cs] = MfmaChain<16>(ap, 4, B816 + 64 + lq * 16 + ix * 8 + l16, 64);
      else if (C == 32) acc[cs] = MfmaChain32L<false>(T.t32_lo, T.t32_hi, (ix * 8 + l16) * 4 + lq, ap, 4);
      else acc[cs] = MfmaChain64L<false>(T.t64, (ix * 8 + l16) * 4 + lq, ap, 4);
    }
  }
  // the rest: two adjacent rows per lane
  const int y = y0 + (lane & 7) * 2, cc = lane >> 3;
  const uint32_t info = ci[(y >> 3) * 8 + cc];
  const bool valu = CellValid(info) && !MfmaCols(ci[(y >> 4) * 16 + (cc >> 1) * 2], ci[(y >> 4) * 16 + 8 + (cc >> 1) * 2]);
  float a0[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (valu) {
    const int ix = CellIx(info), lcx = CellLog2Cx(info);
    const int C = 8 << lcx;
    const float* in = cfc + y * kLP + (cc - ix) * 8;
    if (C == 8) {
#pragma unroll 2
      for (int k = 0; k < 8; k++) { const float v0 = in[k], v1 = in[k + kLP]; JXL_IDCT_STEP(B816 + k * 8, v0, v1) }
    } else if (C == 16) {
      const float* B = B816 + 64 + ix * 8;
#pragma unroll 2
      for (int k = 0; k < 16; k++) { const float v0 = in[k], v1 = in[k + kLP]; JXL_IDCT_STEP(B + k * 16, v0, v1) }
    } else {
      const float* B = Bl + BasisAllOffset(C) + ix * 8;
      for (int k = 0; k < C; k++) { const float v0 = in[k], v1 = in[k + kLP]; JXL_IDCT_STEP(B + k * C, v0, v1) }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int cs = 0; cs < 4; cs++)
    if (m[cs]) {
      float* o = cfc + (y0 + 4 * lq) * kLP + cs * 16 + l16;
      o[0] = acc[cs].x; o[kLP] = acc[cs].y; o[2 * kLP] = acc[cs].z; o[3 * kLP] = acc[cs].w;
    }
  if (valu) {
#pragma unroll
    for (int j = 0; j < 8; j++) { cfc[y * kLP + cc * 8 + j] = a0[j]; cfc[(y + 1) * kLP + cc * 8 + j] = a1[j]; }
  }
}

// Copy-out of the row band the horizontal pass left in this wavefront's hands (no other wavefront wrote it: a wavefront fence is
// enough), 16 bytes per lane, clipped to the padded frame.
__device__ __forceinline__ void ReconCopyOut(const DevImage& im, int tx, int ty) {
  const ReconTile T;
  const ReconLane me;
  const int lane = me.lane, tw = me.tw, c = ChannelOfTeam(me.team);
  const float* const cfc = T.cfc3 + me.team * kTileF;
  const int wp = im.wp, hp = im.hp;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int l16 = lane & 15, lq = lane >> 4;
  float* dst = im.xyb[c];
  const int x4 = l16 * 4;
  const int gx = tx * kTS + x4;
#pragma unroll
  for (int it = 0; it < 4; it++) {
    const int yl = tw * 16 + lq + 4 * it;
    const int gy = ty * kTS + yl;
    const float* r = cfc + yl * kLP + x4;
    const float4 o = make_float4(r[0], r[1], r[2], r[3]);
    if (gx < wp && gy < hp) *(float4*)(dst + (size_t)gy * wp + gx) = o;
  }
}

// One workgroup per 64x64 tile, all three channels (12 wavefronts: team t = wave / 4 owns channel Y, X, B; inside a team the four
// wavefronts split the tile as the one-channel version did): dequantisation with chroma from luma, LF -> LLF, both IDCT passes in
// LDS.  Tiles that hold part of a varblock larger than the tile, or a special 8x8 transform, are appended to a per-image list for
// the generic kernels.
//   * three 64x65 tiles: both IDCT passes run IN PLACE.  The vertical pass gives a wavefront the column stripe [16w, 16w+16) of
//     its channel (everything a stripe's outputs depend on lies in the same columns), the horizontal pass the row band
//     [16w, 16w+16); a wavefront fetches all its operands before it stores, so no workgroup barrier is needed inside a pass, and
//     the copy-out of a row band needs only that wavefront.
//   * the per-cell set-up (cell info, scale, table pointers, entry-list prefixes of the three channels) is done once per tile by
//     wavefront 0; LLF of channel t is computed by the first wavefront of team t with lane shuffles while the others scatter.
//   * 1 / v through v_rcp_f32 (1 ulp; the term is a bias correction <= 0.15 / |v|).
// The 7 of the launch bound is a register cap, not residency: 74 768 bytes of LDS let two workgroups onto a CU, six wavefronts per
// SIMD, whatever the registers.  It keeps the allocator at the 72 VGPRs this kernel compiled to as one body (under a bound of 6 the
// same code cut into phase functions takes 74).  A change that needs up to 80 VGPRs can go back to 6 at no cost in residency.
__global__ __launch_bounds__(768, 7) void recon_tile_kernel(const DevImage* __restrict__ imgs, const float* basis_all, const float* basis_small,
                                                             const float* llf_scale, const float* basis_mfma) {
  JXL_PIXEL_PRIO();
  const ReconTile T;
  const DevImage& im = imgs[blockIdx.y];
  const int tile = blockIdx.x;
  if (tile >= im.wt * im.ht) return;
  const int tid = threadIdx.x;
  const int tx = tile % im.wt, ty = tile / im.wt;
  if (ty < im.dec_gy0 * 4 || ty >= im.dec_gy1 * 4) return;   // outside the decoded band (4 tile rows per group row)
  // the tiles start as zeros: only non-zero coefficients exist in the entry lists
  {
    float4* z = (float4*)T.cfc3;
    for (int i = tid; i < 3 * kTileF / 4; i += 768) z[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // wavefront 0 prepares the cells, the next ones stage the 8- / 16-point bases and the 32-point matrix-core table
  int bad = 0;
  if (tid < 64) {
    bad = ReconCellSetup(im, tx, ty);
  } else if (tid < 64 + 320) {
    T.B816[tid - 64] = basis_all[tid - 64];   // basis_all holds N = 8 at offset 0 and N = 16 at offset 64
  } else if (tid < 64 + 320 + 256) {
    const int i = tid - (64 + 320);         // 16-byte piece i of the 32-point table: run (n, q) = i >> 1, half i & 1
    const float4 v = ((const float4*)basis_mfma)[i];
    if (i & 1) T.t32_hi[i >> 1] = v; else T.t32_lo[i >> 1] = v;
  }
  if (im.num_passes > 1) bad = 1;   // progressive frames: the passes' entries are summed as integers first (expand kernels, generic path)
  if (__syncthreads_or(bad)) {
    if (tid == 0) im.tile_list[atomicAdd(&im.status[1], 1u)] = (uint32_t)tile;
    return;
  }
  if (T.ctot[3]) {   // the tile holds a 64-point varblock: stage that table (16 KB; the barrier before the passes covers it)
    for (int i = tid; i < 1024; i += 768) T.t64[(i & 3) * 256 + (i >> 2)] = ((const float4*)(basis_mfma + 1024))[i];
  }
  if (ReconLane().tw == 0) ReconLlf(im, tx, ty, basis_small, llf_scale);
  ReconScatter(im, tx, ty);
  __syncthreads();
  ReconVerticalPass(basis_all);
  __syncthreads();
  ReconHorizontalPass(basis_all);
  ReconCopyOut(im, tx, ty);
}

// ------------------------------------------------------------------ LDS-tiled loop filters
// kStage: 0 Gaborish, 1 EPF pass 0, 2 EPF pass 1, 3 EPF pass 2.  Tile = 64 x 32 output pixels.
template <int kStage>
__global__ __launch_bounds__(256) void filter_tile_kernel(const DevImage* __restrict__ imgs) {
  JXL_PIXEL_PRIO();
  constexpr int TW = 64, TH = 32;
  constexpr int HALO = kStage == 0 ? 1 : (kStage == 1 ? 3 : (kStage == 2 ? 2 : 1));
  constexpr int LW = TW + 2 * HALO, LH = TH + 2 * HALO;
  __shared__ float t[3][LH][LW + 1];
  const DevImage& im = imgs[blockIdx.y];
  if (!im.stage_on[kStage]) return;
  const int w = im.w, h = im.h, wp = im.wp;
  const int tiles_x = (w + TW - 1) / TW, tiles_y = (h + TH - 1) / TH;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int x0 = tx * TW, y0 = ty * TH;
  // Band decode: the last stage writes exactly the band; earlier stages also produce the rows later stages read (<= 8)
  const bool final_stage = im.final_stage == kStage;
  const int row_lo = final_stage ? im.band_y0 : max(0, im.band_y0 - 8), row_hi = final_stage ? im.band_y1 : min(h, im.band_y1 + 8);
  if (y0 + TH <= row_lo || y0 >= row_hi) return;
  const float* in0 = im.stage_in[kStage][0];
  const float* in1 = im.stage_in[kStage][1];
  const float* in2 = im.stage_in[kStage][2];
  // staged with unconditional (clamped-index) loads in unrolled batches so that a thread's fetches overlap
  constexpr int kLoadIters = (LW * LH + 255) / 256;
#pragma unroll
  for (int it = 0; it < kLoadIters; it++) {
    const int e0 = threadIdx.x + it * 256;
    const int e = e0 < LW * LH ? e0 : LW * LH - 1;
    const int ly = e / LW, lx = e % LW;
    const size_t g = (size_t)ReflectIndex(y0 - HALO + ly, h) * wp + ReflectIndex(x0 - HALO + lx, w);
    const float v0 = in0[g], v1 = in1[g], v2 = in2[g];
    t[0][ly][lx] = v0;
    t[1][ly][lx] = v1;
    t[2][ly][lx] = v2;
  }
  __syncthreads();
#pragma unroll 2
  for (int e = threadIdx.x; e < TW * TH; e += 256) {
    const int ly = e / TW, lx = e % TW;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= w || y < row_lo || y >= row_hi) continue;
    const int cy = ly + HALO, cx = lx + HALO;
    float o0, o1, o2;
    if (kStage == 0) {
      float o[3];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        o[c] = t[c][cy][cx] * im.gab_w[c][0] +
               (t[c][cy - 1][cx] + t[c][cy + 1][cx] + t[c][cy][cx - 1] + t[c][cy][cx + 1]) * im.gab_w[c][1] +
               (t[c][cy - 1][cx - 1] + t[c][cy - 1][cx + 1] + t[c][cy + 1][cx - 1] + t[c][cy + 1][cx + 1]) * im.gab_w[c][2];
      }
      o0 = o[0]; o1 = o[1]; o2 = o[2];
    } else {
      constexpr int kNoff = kStage == 1 ? 12 : 4;
      constexpr int kNplus = kStage == 3 ? 1 : 5;
      const int off0[12][2] = {{-2, 0}, {-1, -1}, {-1, 0}, {-1, 1}, {0, -2}, {0, -1}, {0, 1}, {0, 2}, {1, -1}, {1, 0}, {1, 1}, {2, 0}};
      const int off1[4][2] = {{-1, 0}, {0, -1}, {0, 1}, {1, 0}};
      const int plus[5][2] = {{0, 0}, {-1, 0}, {1, 0}, {0, -1}, {0, 1}};
      const float is = im.inv_sigma[(size_t)(y >> 3) * im.w8 + (x >> 3)];
      o0 = t[0][cy][cx]; o1 = t[1][cy][cx]; o2 = t[2][cy][cx];
      if (!(is < -3.90524291751269967465540850526868f)) {
        const float sm = kStage == 1 ? im.epf_pass0_sigma_scale : (kStage == 2 ? 1.0f : im.epf_pass2_sigma_scale);
        const bool border = ((x & 7) == 0) || ((x & 7) == 7) || ((y & 7) == 0) || ((y & 7) == 7);
        const float inv = is * (border ? sm * im.epf_border_sad_mul : sm);
        float wsum = 1.0f;
#pragma unroll
        for (int k = 0; k < kNoff; k++) {
          const int dy = kStage == 1 ? off0[k][0] : off1[k][0], dx = kStage == 1 ? off0[k][1] : off1[k][1];
          float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
          for (int p = 0; p < kNplus; p++) {
            const int ay = cy + plus[p][0], ax = cx + plus[p][1];
            s0 += fabsf(t[0][ay][ax] - t[0][ay + dy][ax + dx]);
            s1 += fabsf(t[1][ay][ax] - t[1][ay + dy][ax + dx]);
            s2 += fabsf(t[2][ay][ax] - t[2][ay + dy][ax + dx]);
          }
          const float sad = s0 * im.epf_channel_scale[0] + s1 * im.epf_channel_scale[1] + s2 * im.epf_channel_scale[2];
          const float wt = fmaxf(0.0f, 1.0f + sad * inv);
          wsum += wt;
          o0 += wt * t[0][cy + dy][cx + dx];
          o1 += wt * t[1][cy + dy][cx + dx];
          o2 += wt * t[2][cy + dy][cx + dx];
        }
        const float iw = 1.0f / wsum;
        o0 *= iw; o1 *= iw; o2 *= iw;
      }
    }
    if (final_stage) {
      WritePixel(im, x, y, o0, o1, o2);
    } else {
      const size_t g = (size_t)y * wp + x;
      im.stage_out[kStage][0][g] = o0;
      im.stage_out[kStage][1][g] = o1;
      im.stage_out[kStage][2][g] = o2;
    }
  }
}

// Gaborish + EPF pass 1 (the only pass of epf_iters == 1) + XYB -> output samples in one kernel, WITHOUT LDS: a wavefront owns a
// strip of 256 columns (64 quads of 4 pixels; the outer quad each side is halo, 248 columns are output) and walks
// down a segment of rows.  Every lane keeps the rolling windows of its quad in registers - two input rows with their horizontal
// neighbour sums, three Gaborish rows, three rows of vertical and of horizontal channel-weighted differences - and gets its
// horizontal neighbours from the lanes beside it by DPP wave shifts (v_mov_dpp wave_shr / wave_shl: one VALU op, no LDS round trip).
// Per input row a lane issues three 16-byte loads (256 contiguous bytes per group and plane), one row ahead of their use; per
// output row one 16-byte store.  The LDS-tiled version read ~75 LDS words per pixel (37 % of its LDS cycles bank conflicts) and
// re-read a 38 x 40 footprint per 32 x 32 tile (1.48x); this one reads 64 / 56 x 70 / 64 = 1.25x and is bound by its VALU work.
constexpr int kStripLanes = 64;                    // lanes of a strip: a whole wavefront (DPP wave shifts cross the rows of 16)
constexpr int kStripOut = 4 * (kStripLanes - 2);   // output columns of a strip: every lane's quad but the two halo quads at its ends (248;
                                                   // with strips of one DPP row - 16 lanes, 56 of 64 columns - a seventh of the work was halo)
constexpr int kGroupsPerWg = 256 / kStripLanes;
constexpr int kSegRows = 128;    // output rows of a segment (+ 3 halo rows each side)
__device__ __forceinline__ float DppFromLeft(float v) {    // value of lane - 1 inside the row of 16 (lane 0: 0)
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138 /* wave_shr:1 */, 0xF, 0xF, true));
}
__device__ __forceinline__ float DppFromRight(float v) {   // value of lane + 1 inside the row of 16 (lane 15: 0)
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130 /* wave_shl:1 */, 0xF, 0xF, true));
}
__device__ __forceinline__ F4 ShiftFromLeft(F4 v) { return F4{DppFromLeft(v.w), v.x, v.y, v.z}; }      // element x - 1
__device__ __forceinline__ F4 ShiftFromRight(F4 v) { return F4{v.y, v.z, v.w, DppFromRight(v.x)}; }    // element x + 1
__device__ __forceinline__ F4 ShiftFromLeft2(F4 v) { return F4{DppFromLeft(v.z), DppFromLeft(v.w), v.x, v.y}; }   // element x - 2
__device__ __forceinline__ F4 Abs(F4 v) { return F4{fabsf(v.x), fabsf(v.y), fabsf(v.z), fabsf(v.w)}; }
// The two-pixels-per-lane forms (filter_stream_pairs_kernel, filter_stream2_pairs_kernel) run the same arithmetic on F2
typedef float __attribute__((ext_vector_type(2))) F2;
typedef unsigned __attribute__((ext_vector_type(2))) U2v;
__device__ __forceinline__ F2 ShiftFromLeft(F2 v) { return F2{DppFromLeft(v.y), v.x}; }
__device__ __forceinline__ F2 ShiftFromRight(F2 v) { return F2{v.y, DppFromRight(v.x)}; }
__device__ __forceinline__ F2 ShiftFromLeft2(F2 v) { return F2{DppFromLeft(v.x), DppFromLeft(v.y)}; }
__device__ __forceinline__ F2 Abs(F2 v) { return F2{fabsf(v.x), fabsf(v.y)}; }

// The lane's pixels (V = F4: a quad, F2: a pair) of one row of the three planes
template <typename V> struct RowOf { V c[3]; };
template <typename V> constexpr int kLanePixels = sizeof(V) / sizeof(float);
typedef RowOf<F4> Row3;
typedef RowOf<F2> PairRow;
#define JXL_GLOBAL __attribute__((address_space(1)))
// Quad (X .. X + 3) of row y of the three planes; rows and columns outside the frame are mirrored like the unfused stages do.
__device__ __forceinline__ Row3 LoadRow3(const JXL_GLOBAL float* p0, const JXL_GLOBAL float* p1, const JXL_GLOBAL float* p2, int X, int y, int w, int h,
                                         int wp, bool interior) {
  const int yy = ReflectIndex(y, h);   // rows y0 - 3 .. y1 + 2: more than one reflection for h <= 2
  Row3 r;
  if (interior) {
    const size_t g = (size_t)yy * wp + X;
    r.c[0] = *(const JXL_GLOBAL F4*)(p0 + g); r.c[1] = *(const JXL_GLOBAL F4*)(p1 + g); r.c[2] = *(const JXL_GLOBAL F4*)(p2 + g);
  } else {
    const size_t g = (size_t)yy * wp;
    const int x0 = ReflectIndex(X, w), x1 = ReflectIndex(X + 1, w), x2 = ReflectIndex(X + 2, w), x3 = ReflectIndex(X + 3, w);
    r.c[0] = F4{p0[g + x0], p0[g + x1], p0[g + x2], p0[g + x3]};
    r.c[1] = F4{p1[g + x0], p1[g + x1], p1[g + x2], p1[g + x3]};
    r.c[2] = F4{p2[g + x0], p2[g + x1], p2[g + x2], p2[g + x3]};
  }
  return r;
}
// Rolling windows of one lane, as four slots each, indexed by (row & 3) with COMPILE-TIME phases (the row loop is unrolled by four):
// no register moves to shift a window.  in / s: input rows and their horizontal neighbour sums; g: Gaborish rows; dv / dh: vertical /
// horizontal channel-weighted differences of Gaborish rows; hd: dv[x-1] + dv[x+1].
template <typename V> struct Windows {
  RowOf<V> in[4], s[4], g[4];
  V dv[4], dh[4], hd[4];
};
typedef Windows<F4> StreamState;
typedef Windows<F2> PairState;
template <typename V>
__device__ __forceinline__ void ZeroWindows(Windows<V>& st) {
  const V zero = V(0.f);
#pragma unroll
  for (int i = 0; i < 4; i++) {
#pragma unroll
    for (int c = 0; c < 3; c++) { st.in[i].c[c] = zero; st.s[i].c[c] = zero; st.g[i].c[c] = zero; }
    st.dv[i] = zero; st.dh[i] = zero; st.hd[i] = zero;
  }
}
// What the arithmetic of a Gaborish + EPF-1 row needs besides the windows; both forms' constants start with it
struct RowConst {
  float gw0[3], gw1[3], gw2[3], cs[3], bsm;
  int y0, y1;   // output rows of the lane's segment
};
__device__ __forceinline__ void FillRowConst(const DevImage& im, RowConst& k) {
  const bool no_gab = im.stream_no_gab != 0;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    // without Gaborish the kernel's weights are the identity: x * 1 + a * 0 + b * 0 is x exactly for finite planes
    k.gw0[c] = no_gab ? 1.0f : im.gab_w[c][0]; k.gw1[c] = no_gab ? 0.0f : im.gab_w[c][1]; k.gw2[c] = no_gab ? 0.0f : im.gab_w[c][2];
    k.cs[c] = im.epf_channel_scale[c];
  }
  k.bsm = im.epf_border_sad_mul;
}
// The lane's vector of 1 / sigma terms: inv_b for a first / last pixel that lies in a block-border column, inv_in elsewhere
template <typename V>
__device__ __forceinline__ V BorderInv(float inv_in, float inv_b, bool xb_first, bool xb_last) {
  V inv = V(inv_in);
  inv[0] = xb_first ? inv_b : inv_in; inv[kLanePixels<V> - 1] = xb_last ? inv_b : inv_in;
  return inv;
}

// The arithmetic of one input row r = y + 3 (phase P = (r - first row) & 3), for any lane vector (used by the two-pixel form; the four-pixel
// form keeps a copy, see StreamRow): Gaborish row r - 1, differences, and, when
// y is a row of the lane's segment (the function then returns true), EPF pass 1 of the output row y into o[].  `cur`: input row r;
// `is`: 1 / sigma of row y's cell; xb_first / xb_last: the lane's first / last pixel lies in the first / last column of an 8x8 block.
// (Operand order and grouping of the floating-point expressions are part of the result: leave them as they are.)
template <int P, typename V>
__device__ __forceinline__ bool GabEpf1Row(const RowOf<V>& cur, Windows<V>& st, const RowConst& k, float is, int y, bool xb_first, bool xb_last,
                                           V o[3]) {
  constexpr int s0 = P, s1 = (P + 1) & 3, s2 = (P + 2) & 3, s3 = (P + 3) & 3;   // slots of rows r (= r - 4), r - 3, r - 2, r - 1
  const V zero = V(0.f);
  V dhn = zero, dvn = zero;
  st.in[s0] = cur;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    st.s[s0].c[c] = ShiftFromLeft(cur.c[c]) + ShiftFromRight(cur.c[c]);
    // Gaborish of row r - 1 from input rows r - 2, r - 1, r
    const V gn = st.in[s3].c[c] * k.gw0[c] + ((st.in[s2].c[c] + cur.c[c]) + st.s[s3].c[c]) * k.gw1[c] + (st.s[s2].c[c] + st.s[s0].c[c]) * k.gw2[c];
    dhn += Abs(gn - ShiftFromRight(gn)) * k.cs[c];      // dh[r-1][x] = sum_c scale_c |gab[x] - gab[x + 1]|
    dvn += Abs(st.g[s2].c[c] - gn) * k.cs[c];            // dv[r-2][x] = sum_c scale_c |gab[r-2] - gab[r-1]|
    st.g[s3].c[c] = gn;
  }
  // now: g[s0] = gab[r-4], g[s1] = gab[r-3], g[s2] = gab[r-2]; dv[s3] = dv[r-5], dv[s0] = dv[r-4], dv[s1] = dv[r-3]; dh[s0..s2] = dh[r-4..r-2]
  const V dv0 = st.dv[s3], dv1 = st.dv[s0], dv2 = st.dv[s1];
  const V hd2 = ShiftFromLeft(dv2) + ShiftFromRight(dv2);    // dv[y][x-1] + dv[y][x+1]
  const V hd1 = st.hd[s0];
  const bool output_row = y >= k.y0 && y < k.y1;   // uniform over the wavefront (four pixels per lane: except in a shorter last segment)
  if (output_row) {
    // EPF pass 1 of row y: neighbours up / left / right / down, SAD over the plus-shaped support
    const V dh0 = st.dh[s0], dh1 = st.dh[s1], dh2 = st.dh[s2];
    const V a = dv1 + dv2;
    const V sad_u = a + dv0 + hd1, sad_d = a + dvn + hd2;
    const V vh = dh0 + dh1 + dh2;
    const V sad_r = vh + (ShiftFromLeft(dh1) + ShiftFromRight(dh1));
    const V sad_l = ShiftFromLeft(vh) + (ShiftFromLeft2(dh1) + dh1);
    const bool yb = ((y & 7) == 0) || ((y & 7) == 7);
    const V inv = BorderInv<V>(is * (yb ? k.bsm : 1.0f), is * k.bsm, xb_first, xb_last);
    const bool skip = is < -3.90524291751269967465540850526868f;
    V wu, wl, wr, wd, iw;
#pragma unroll
    for (int j = 0; j < kLanePixels<V>; j++) {
      wu[j] = fmaxf(0.f, 1.0f + sad_u[j] * inv[j]); wl[j] = fmaxf(0.f, 1.0f + sad_l[j] * inv[j]);
      wr[j] = fmaxf(0.f, 1.0f + sad_r[j] * inv[j]); wd[j] = fmaxf(0.f, 1.0f + sad_d[j] * inv[j]);
      iw[j] = __builtin_amdgcn_rcpf(1.0f + wu[j] + wl[j] + wr[j] + wd[j]);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const V g1 = st.g[s1].c[c];
      const V f = (g1 + wu * st.g[s0].c[c] + wl * ShiftFromLeft(g1) + wr * ShiftFromRight(g1) + wd * st.g[s2].c[c]) * iw;
      o[c] = skip ? g1 : f;
    }
  }
  st.dv[s2] = dvn;   // dv[r-2]
  st.dh[s3] = dhn;   // dh[r-1]
  st.hd[s1] = hd2;   // of dv[r-3]: next row's hd1
  return output_row;
}
// The arithmetic of one row y of the second EPF iteration, for both forms: three rows of the first iteration's output, four neighbours,
// a one-pixel SAD.  cs: channel scales; sm / smb: the iteration's sigma scale, and the same times the border multiplier.
template <typename V>
__device__ __forceinline__ void Epf2Row(const RowOf<V>& prev, const RowOf<V>& cur, const RowOf<V>& next, const float (&cs)[3], float sm, float smb,
                                        float is, int y, bool xb_first, bool xb_last, V o[3]) {
  const V zero = V(0.f);
  V su = zero, sd = zero, sl = zero, sr = zero;
  V lft[3], rgt[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    lft[c] = ShiftFromLeft(cur.c[c]); rgt[c] = ShiftFromRight(cur.c[c]);
    su += Abs(cur.c[c] - prev.c[c]) * cs[c]; sd += Abs(cur.c[c] - next.c[c]) * cs[c];
    sl += Abs(cur.c[c] - lft[c]) * cs[c]; sr += Abs(cur.c[c] - rgt[c]) * cs[c];
  }
  const bool yb = ((y & 7) == 0) || ((y & 7) == 7);
  const V inv = BorderInv<V>(is * (yb ? smb : sm), is * smb, xb_first, xb_last);
  const bool skip = is < -3.90524291751269967465540850526868f;
  V wu, wl, wr, wd, iw;
#pragma unroll
  for (int j = 0; j < kLanePixels<V>; j++) {
    wu[j] = fmaxf(0.f, 1.0f + su[j] * inv[j]); wl[j] = fmaxf(0.f, 1.0f + sl[j] * inv[j]);
    wr[j] = fmaxf(0.f, 1.0f + sr[j] * inv[j]); wd[j] = fmaxf(0.f, 1.0f + sd[j] * inv[j]);
    iw[j] = __builtin_amdgcn_rcpf(1.0f + wu[j] + wl[j] + wr[j] + wd[j]);
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const V f = (cur.c[c] + wu * prev.c[c] + wl * lft[c] + wr * rgt[c] + wd * next.c[c]) * iw;
    o[c] = skip ? cur.c[c] : f;
  }
}

// Which strip and segment a lane works on (filter_stream_kernel decodes the same way, in its own words: see StreamRow).  A wavefront is a strip of 64 lanes with `px` pixels each, of
// which `halo` lanes at each end only feed their neighbours: out_cols = px * (64 - 2 * halo) output columns.  A strip walks down a
// segment of kSegRows rows of the band [band_lo, band_hi).
struct StripTask {
  bool stores;      // this lane stores its pixels (a lane of a wavefront with a task of its own, not a halo lane, inside the frame)
  int q;            // the lane's index in the strip
  int X, y0, y1;    // first column of the lane's pixels (may lie outside the frame); rows of the segment
};
// `wave`: the wavefront's index in the workgroup.  False: the whole workgroup is past the end.  Every lane of a workgroup with a task stays
// in the row loop (DPP reads neighbouring lanes): wavefronts past the end repeat the last task and store nothing.
__device__ __forceinline__ bool GetStripTask(int wave, int w, int band_lo, int band_hi, int out_cols, int halo, int px, StripTask& t) {
  const int strips = (w + out_cols - 1) / out_cols;
  const int segs = (band_hi - band_lo + kSegRows - 1) / kSegRows;
  if ((int)blockIdx.x * kGroupsPerWg >= strips * segs) return false;
  const int gidx = blockIdx.x * kGroupsPerWg + wave;
  const bool task = gidx < strips * segs;
  const int gi = task ? gidx : strips * segs - 1;
  const int strip = gi % strips, seg = gi / strips;
  t.q = threadIdx.x & (kStripLanes - 1);
  t.X = strip * out_cols - halo * px + px * t.q;
  t.y0 = band_lo + seg * kSegRows; t.y1 = min(t.y0 + kSegRows, band_hi);
  t.stores = task && t.q >= halo && t.q <= kStripLanes - 1 - halo && t.X < w;
  return true;
}

// Alpha of the quad at p, packed (the plain layouts of the four-pixel kernels)
__device__ __forceinline__ uint32_t LoadAlphaQuad(const JXL_GLOBAL uint8_t* ap) {
  return (uint32_t)ap[0] | (uint32_t)ap[1] << 8 | (uint32_t)ap[2] << 16 | (uint32_t)ap[3] << 24;
}
// The output block of the four-pixel kernels (StreamRow holds its own copy): quad X .. X + 3 of row y.  Whole RGBA quads of the plain layouts (`fast`) leave as one
// 16-byte store with the packed alpha quad `al`; everything else pixel by pixel through the general writer.
__device__ __forceinline__ void StoreQuad(const DevImage& im, const F4 (&o)[3], uint32_t al, int X, int y, int w, bool fast) {
  if (fast) {
    typedef unsigned __attribute__((ext_vector_type(4))) U4v;
    U4v px;
    px.x = PixelToRgba8(im, o[0].x, o[1].x, o[2].x, al & 0xFF);
    px.y = PixelToRgba8(im, o[0].y, o[1].y, o[2].y, (al >> 8) & 0xFF);
    px.z = PixelToRgba8(im, o[0].z, o[1].z, o[2].z, (al >> 16) & 0xFF);
    px.w = PixelToRgba8(im, o[0].w, o[1].w, o[2].w, al >> 24);
    *(JXL_GLOBAL U4v*)((JXL_GLOBAL uint8_t*)im.out + ((size_t)(y - im.band_y0) * w + X) * 4) = px;
  } else {
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
      if (X + j >= w) break;
      const uint32_t aj = !im.has_alpha ? 0u : LoadAlpha(im, (size_t)y * w + X + j);   // (the packed quad `al` is only valid for whole quads)
      const float ox = j == 0 ? o[0].x : (j == 1 ? o[0].y : (j == 2 ? o[0].z : o[0].w));
      const float oy = j == 0 ? o[1].x : (j == 1 ? o[1].y : (j == 2 ? o[1].z : o[1].w));
      const float ob = j == 0 ? o[2].x : (j == 1 ? o[2].y : (j == 2 ? o[2].z : o[2].w));
      WritePixelGeneral(im, X + j, y, ox, oy, ob, aj);
    }
  }
}

struct StreamConst {
  const JXL_GLOBAL float *in0, *in1, *in2, *inv_sigma;
  const JXL_GLOBAL uint8_t* alpha;
  float gw0[3], gw1[3], gw2[3], cs[3], bsm;
  int X, w, h, wp, w8, y0, y1, r_end, cellx, xa;
  bool interior, stores, full_quad, plain, xb0, xb3;
  JXL_GLOBAL float *f0, *f1, *f2;   // two EPF iterations: the first one's rows leave as f32 planes (filter_stream2_kernel reads them)
  bool to_float;
};

// One input row r (phase P = (r - first row) & 3) of the four-pixel form: Gaborish row r - 1, differences, and the output row r - 3.
// The arithmetic is GabEpf1Row's, written out a second time ON PURPOSE, like the set-up in filter_stream_kernel below (task decoding,
// weights, zeroed windows, output block): this kernel sits at 251 registers, two wavefronts per SIMD, and every way of calling the shared
// pieces tried so far moved its allocation (244 .. 256 registers, one with scratch) - through GabEpf1Row it measured 1.3 % slower
// (profiles/shared_bodies_filter_layouts.txt).  As written here its code is the same instruction for instruction as before the bodies
// were shared.  A change to the filter goes into GabEpf1Row AND here; tests/test_gpu_parity.py holds the two forms to identical bytes.
template <int P>
__device__ __forceinline__ void StreamRow(const DevImage& im, const StreamConst& k, StreamState& st, Row3& next, int r) {
  constexpr int s0 = P, s1 = (P + 1) & 3, s2 = (P + 2) & 3, s3 = (P + 3) & 3;   // slots of rows r (= r - 4), r - 3, r - 2, r - 1
  const Row3 cur = next;
  next = LoadRow3(k.in0, k.in1, k.in2, k.X, min(r + 1, k.r_end - 1), k.w, k.h, k.wp, k.interior);
  // operands of the output row y = r - 3, requested a whole row of arithmetic ahead of their use
  const int y = r - 3;
  const int yc = min(max(y, 0), k.h - 1);
  const float is = k.inv_sigma[(size_t)(yc >> 3) * k.w8 + k.cellx];
  uint32_t al = 0xFFFFFFFFu;
  if (im.has_alpha && k.plain) al = LoadAlphaQuad(k.alpha + (size_t)yc * k.w + k.xa);
  const F4 zero = {0.f, 0.f, 0.f, 0.f};
  F4 dhn = zero, dvn = zero;
  st.in[s0] = cur;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    st.s[s0].c[c] = ShiftFromLeft(cur.c[c]) + ShiftFromRight(cur.c[c]);
    // Gaborish of row r - 1 from input rows r - 2, r - 1, r
    const F4 gn = st.in[s3].c[c] * k.gw0[c] + ((st.in[s2].c[c] + cur.c[c]) + st.s[s3].c[c]) * k.gw1[c] + (st.s[s2].c[c] + st.s[s0].c[c]) * k.gw2[c];
    dhn += Abs(gn - ShiftFromRight(gn)) * k.cs[c];      // dh[r-1][x] = sum_c scale_c |gab[x] - gab[x + 1]|
    dvn += Abs(st.g[s2].c[c] - gn) * k.cs[c];            // dv[r-2][x] = sum_c scale_c |gab[r-2] - gab[r-1]|
    st.g[s3].c[c] = gn;
  }
  // now: g[s0] = gab[r-4], g[s1] = gab[r-3], g[s2] = gab[r-2]; dv[s3] = dv[r-5], dv[s0] = dv[r-4], dv[s1] = dv[r-3]; dh[s0..s2] = dh[r-4..r-2]
  const F4 dv0 = st.dv[s3], dv1 = st.dv[s0], dv2 = st.dv[s1];
  const F4 hd2 = ShiftFromLeft(dv2) + ShiftFromRight(dv2);    // dv[y][x-1] + dv[y][x+1]
  const F4 hd1 = st.hd[s0];
  if (y >= k.y0 && y < k.y1) {   // uniform over the wavefront except for its groups in a shorter last segment
    // EPF pass 1 of row y: neighbours up / left / right / down, SAD over the plus-shaped support
    const F4 dh0 = st.dh[s0], dh1 = st.dh[s1], dh2 = st.dh[s2];
    const F4 a = dv1 + dv2;
    const F4 sad_u = a + dv0 + hd1, sad_d = a + dvn + hd2;
    const F4 vh = dh0 + dh1 + dh2;
    const F4 sad_r = vh + (ShiftFromLeft(dh1) + ShiftFromRight(dh1));
    const F4 sad_l = ShiftFromLeft(vh) + (ShiftFromLeft2(dh1) + dh1);
    const bool yb = ((y & 7) == 0) || ((y & 7) == 7);
    const float inv_in = is * (yb ? k.bsm : 1.0f), inv_b = is * k.bsm;
    const F4 inv = {k.xb0 ? inv_b : inv_in, inv_in, inv_in, k.xb3 ? inv_b : inv_in};
    const bool skip = is < -3.90524291751269967465540850526868f;
    F4 wu, wl, wr, wd, iw;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      wu[j] = fmaxf(0.f, 1.0f + sad_u[j] * inv[j]); wl[j] = fmaxf(0.f, 1.0f + sad_l[j] * inv[j]);
      wr[j] = fmaxf(0.f, 1.0f + sad_r[j] * inv[j]); wd[j] = fmaxf(0.f, 1.0f + sad_d[j] * inv[j]);
      iw[j] = __builtin_amdgcn_rcpf(1.0f + wu[j] + wl[j] + wr[j] + wd[j]);
    }
    F4 o[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const F4 g1 = st.g[s1].c[c];
      const F4 f = (g1 + wu * st.g[s0].c[c] + wl * ShiftFromLeft(g1) + wr * ShiftFromRight(g1) + wd * st.g[s2].c[c]) * iw;
      o[c] = skip ? g1 : f;
    }
    if (k.stores && k.to_float) {
      // (the planes are padded to whole 8x8 cells: a quad that starts inside the frame ends inside the plane)
      const size_t g = (size_t)y * k.wp + k.X;
      *(JXL_GLOBAL F4*)(k.f0 + g) = o[0]; *(JXL_GLOBAL F4*)(k.f1 + g) = o[1]; *(JXL_GLOBAL F4*)(k.f2 + g) = o[2];
    } else if (k.stores) {
      if (k.plain && im.nch_out == 4 && k.full_quad) {
        typedef unsigned __attribute__((ext_vector_type(4))) U4v;
        U4v px;
        px.x = PixelToRgba8(im, o[0].x, o[1].x, o[2].x, al & 0xFF);
        px.y = PixelToRgba8(im, o[0].y, o[1].y, o[2].y, (al >> 8) & 0xFF);
        px.z = PixelToRgba8(im, o[0].z, o[1].z, o[2].z, (al >> 16) & 0xFF);
        px.w = PixelToRgba8(im, o[0].w, o[1].w, o[2].w, al >> 24);
        *(JXL_GLOBAL U4v*)((JXL_GLOBAL uint8_t*)im.out + ((size_t)(y - im.band_y0) * k.w + k.X) * 4) = px;
      } else {
#pragma unroll 1
        for (int j = 0; j < 4; j++) {
          if (k.X + j >= k.w) break;
          const uint32_t aj = !im.has_alpha ? 0u : LoadAlpha(im, (size_t)y * k.w + k.X + j);   // (the packed quad `al` is only valid for whole quads)
          const float ox = j == 0 ? o[0].x : (j == 1 ? o[0].y : (j == 2 ? o[0].z : o[0].w));
          const float oy = j == 0 ? o[1].x : (j == 1 ? o[1].y : (j == 2 ? o[1].z : o[1].w));
          const float ob = j == 0 ? o[2].x : (j == 1 ? o[2].y : (j == 2 ? o[2].z : o[2].w));
          WritePixelGeneral(im, k.X + j, y, ox, oy, ob, aj);
        }
      }
    }
  }
  st.dv[s2] = dvn;   // dv[r-2]
  st.dh[s3] = dhn;   // dh[r-1]
  st.hd[s1] = hd2;   // of dv[r-3]: next row's hd1
}

__global__ __launch_bounds__(256, 2) void filter_stream_kernel(const DevImage* __restrict__ imgs) {
  JXL_PIXEL_PRIO();
  const DevImage& im = imgs[blockIdx.y];
  if (!im.fused_gab_epf1 || (im.stream_pairs & 1)) return;   // (the common layouts run in filter_stream_pairs_kernel)
  StreamConst k;
  k.w = im.w; k.h = im.h; k.wp = im.wp; k.w8 = im.w8;
  const int strips = (k.w + kStripOut - 1) / kStripOut;
  // two EPF iterations: this kernel's rows feed the second iteration, which looks one row up and down
  k.to_float = im.fused_gab_epf1 == 2;
  const int band_lo = k.to_float ? max(0, im.band_y0 - 1) : im.band_y0, band_hi = k.to_float ? min(k.h, im.band_y1 + 1) : im.band_y1;
  const int band_rows = band_hi - band_lo;
  const int segs = (band_rows + kSegRows - 1) / kSegRows;
  if ((int)blockIdx.x * kGroupsPerWg >= strips * segs) return;   // whole workgroup past the end
  // every lane stays in the loop (DPP reads neighbouring lanes); groups past the end repeat the last task and store nothing
  const int gidx = blockIdx.x * kGroupsPerWg + (threadIdx.x / kStripLanes);
  const bool task = gidx < strips * segs;
  const int gi = task ? gidx : strips * segs - 1;
  const int strip = gi % strips, seg = gi / strips;
  const int q = threadIdx.x & (kStripLanes - 1);
  k.X = strip * kStripOut - 4 + 4 * q;           // first column of this lane's quad
  k.y0 = band_lo + seg * kSegRows; k.y1 = min(k.y0 + kSegRows, band_hi);
  k.r_end = k.y1 + 3;
  k.interior = k.X >= 0 && k.X + 3 < k.w;
  k.stores = task && q >= 1 && q <= kStripLanes - 2 && k.X < k.w;
  k.full_quad = k.X + 3 < k.w;
  k.in0 = (const JXL_GLOBAL float*)im.stream_in[0];
  k.in1 = (const JXL_GLOBAL float*)im.stream_in[1];
  k.in2 = (const JXL_GLOBAL float*)im.stream_in[2];
  const bool no_gab = im.stream_no_gab != 0;
  k.inv_sigma = (const JXL_GLOBAL float*)im.inv_sigma;
  k.alpha = (const JXL_GLOBAL uint8_t*)im.alpha;
  k.plain = PlainOutput(im);
  k.f0 = (JXL_GLOBAL float*)im.stream_mid[0]; k.f1 = (JXL_GLOBAL float*)im.stream_mid[1]; k.f2 = (JXL_GLOBAL float*)im.stream_mid[2];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    // without Gaborish the kernel's weights are the identity: x * 1 + a * 0 + b * 0 is x exactly for finite planes
    k.gw0[c] = no_gab ? 1.0f : im.gab_w[c][0]; k.gw1[c] = no_gab ? 0.0f : im.gab_w[c][1]; k.gw2[c] = no_gab ? 0.0f : im.gab_w[c][2];
    k.cs[c] = im.epf_channel_scale[c];
  }
  k.bsm = im.epf_border_sad_mul;
  // block-border columns of the quad: strips start on a multiple of 8, so X = 4 (q - 1) mod 8
  k.xb0 = (q & 1) != 0; k.xb3 = (q & 1) == 0;     // component 0 is column 0 of a block / component 3 is column 7
  k.cellx = min(max(k.X, 0), k.w - 1) >> 3;
  k.xa = min(max(k.X, 0), max(k.w - 4, 0));       // alpha quad (clamped: halo lanes and partial quads never use it)
  StreamState st;
  const F4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; i++) {
#pragma unroll
    for (int c = 0; c < 3; c++) { st.in[i].c[c] = zero; st.s[i].c[c] = zero; st.g[i].c[c] = zero; }
    st.dv[i] = zero; st.dh[i] = zero; st.hd[i] = zero;
  }
  const int r0 = k.y0 - 3;
  Row3 next = LoadRow3(k.in0, k.in1, k.in2, k.X, r0, k.w, k.h, k.wp, k.interior);
  // four rows per trip, unconditionally (rows past the end recompute the last input row and store nothing: y >= y1): with
  // conditional phases the compiler must keep every slot of every window alive across the back edge
  for (int r = r0; r < k.r_end; r += 4) {
    StreamRow<0>(im, k, st, next, r);
    StreamRow<1>(im, k, st, next, r + 1);
    StreamRow<2>(im, k, st, next, r + 2);
    StreamRow<3>(im, k, st, next, r + 3);
  }
}

// ---- The same kernel for the common layouts, TWO pixels per lane --------------------------------------------------------------------
// (even width >= 8; RGBA8 output with an alpha plane, or the f32 rows of a first of two iterations.)  What it changes, and why:
//  * half the window state per lane -> 128 registers instead of 252: four wavefronts per SIMD instead of two, and a wavefront of
//    this kernel still fits on a SIMD that an entropy wavefront of another batch occupies (measured in the pipelined step: with 252
//    registers ONE wavefront fitted beside an entropy wavefront, the kernel ran at half speed whenever the chains overlapped);
//  * buffer addressing (a 128-bit resource in scalar registers + a scalar row offset + the lane's 32-bit byte offset): no per-lane
//    64-bit addresses to compute or keep;
//  * no load sits in a branch: the pair left of column 0 and the pairs right of column w - 1 are pairs inside the frame, mirrored -
//    such a lane loads the pair it mirrors and swaps it.  (With loads in divergent branches the compiler loses count of the loads in
//    flight at the join and waits for ALL of them, the prefetched row included);
//  * the sigma cell and the alpha pair of a row are requested one row ahead, like the input pairs.
// A strip = 128 columns, the outer two pairs each side are halo (the filters reach 3 columns): 120 output columns.
constexpr int kPairOut = 2 * (kStripLanes - 4);
struct PairConst : RowConst {
  __amdgpu_buffer_rsrc_t in0, in1, in2, sigma, alpha, out, f0, f1, f2;
  int w, h, wp, w8, r_end, band_y0;
  uint32_t in_bytes, cell_bytes, alpha_bytes, out_bytes;   // the lane's byte offsets inside a row: mirrored input pair, sigma cell, alpha pair, pair
  bool outside, stores, to_float, use_alpha, xb_lo, xb_hi;
  int bpp;   // bytes per output pixel: 4 RGBA, 3 RGB, 2 gray + alpha, 1 gray
};
struct PairAux { float is; uint32_t al; };
// Two output pixels of a lane (p = R | G << 8 | B << 16 | A << 24 each): 8 bytes RGBA; 6 bytes RGB as three 16-bit stores (the pair starts
// on an even column: 2-byte aligned); gray + alpha as one 32-bit store; gray as one 16-bit store (gray frames: R = G = B)
__device__ __forceinline__ void StorePixelPair(const PairConst& k, uint32_t p0, uint32_t p1, int row) {
  const uint32_t x = k.out_bytes >> 2;   // first column of the pair
  if (k.bpp == 4) {
    U2v px; px.x = p0; px.y = p1;
    __builtin_amdgcn_raw_buffer_store_b64(px, k.out, k.out_bytes, (uint32_t)row * (uint32_t)k.w * 4u, 0);
  } else if (k.bpp == 3) {
    const uint32_t soff = (uint32_t)row * (uint32_t)k.w * 3u, v = x * 3u;
    __builtin_amdgcn_raw_buffer_store_b16((short)(p0 & 0xFFFFu), k.out, v, soff, 0);
    __builtin_amdgcn_raw_buffer_store_b16((short)(((p0 >> 16) & 0xFFu) | ((p1 & 0xFFu) << 8)), k.out, v + 2, soff, 0);
    __builtin_amdgcn_raw_buffer_store_b16((short)((p1 >> 8) & 0xFFFFu), k.out, v + 4, soff, 0);
  } else if (k.bpp == 2) {
    const uint32_t ga = ((p0 >> 8) & 0xFFu) | ((p0 >> 24) << 8) | (((p1 >> 8) & 0xFFu) << 16) | ((p1 >> 24) << 24);
    __builtin_amdgcn_raw_buffer_store_b32(ga, k.out, x * 2u, (uint32_t)row * (uint32_t)k.w * 2u, 0);
  } else {
    __builtin_amdgcn_raw_buffer_store_b16((short)(((p0 >> 8) & 0xFFu) | (((p1 >> 8) & 0xFFu) << 8)), k.out, x, (uint32_t)row * (uint32_t)k.w, 0);
  }
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t PlaneResource(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, 0x7FFFFFFF, 0x00020000);   // raw buffer, no swizzle; the planes are smaller than 2 GB
}
__device__ __forceinline__ PairRow LoadPairRow(const PairConst& k, int y) {
  const int yy = ReflectIndex(y, k.h);   // uniform over the wavefront (the loop stays on the scalar unit); h <= 2 reflects more than once
  const uint32_t row = (uint32_t)yy * (uint32_t)k.wp * 4u;
  PairRow r;
  r.c[0] = __builtin_bit_cast(F2, __builtin_amdgcn_raw_buffer_load_b64(k.in0, k.in_bytes, row, 0));
  r.c[1] = __builtin_bit_cast(F2, __builtin_amdgcn_raw_buffer_load_b64(k.in1, k.in_bytes, row, 0));
  r.c[2] = __builtin_bit_cast(F2, __builtin_amdgcn_raw_buffer_load_b64(k.in2, k.in_bytes, row, 0));
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const F2 v = r.c[c];
    r.c[c] = k.outside ? F2{v.y, v.x} : v;
  }
  return r;
}
__device__ __forceinline__ PairAux LoadPairAux(const PairConst& k, int y) {
  const int yc = min(max(y, 0), k.h - 1);
  PairAux a;
  a.is = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(k.sigma, k.cell_bytes, (uint32_t)(yc >> 3) * (uint32_t)k.w8 * 4u, 0));
  a.al = (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(k.alpha, k.alpha_bytes, (uint32_t)yc * (uint32_t)k.w, 0);
  return a;
}
// One input row r of the two-pixel form: its loads (all the next row reads from memory, a whole row of arithmetic ahead of its use; none
// in a branch) and its stores around GabEpf1Row.
template <int P>
__device__ __forceinline__ void PairStreamRow(const DevImage& im, const PairConst& k, PairState& st, PairRow& next, PairAux& next_aux, int r) {
  const PairRow cur = next;
  const PairAux aux = next_aux;
  next = LoadPairRow(k, min(r + 1, k.r_end - 1));
  next_aux = LoadPairAux(k, r - 2);
  const int y = r - 3;   // the output row
  const uint32_t al = k.use_alpha ? aux.al : 0xFFFFu;
  F2 o[3];
  if (!GabEpf1Row<P>(cur, st, k, aux.is, y, k.xb_lo, k.xb_hi, o)) return;
  if (k.stores) {
    if (k.to_float) {
      const uint32_t row = (uint32_t)y * (uint32_t)k.wp * 4u;
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(U2v, o[0]), k.f0, k.out_bytes, row, 0);
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(U2v, o[1]), k.f1, k.out_bytes, row, 0);
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(U2v, o[2]), k.f2, k.out_bytes, row, 0);
    } else {
      StorePixelPair(k, PixelToRgba8(im, o[0].x, o[1].x, o[2].x, al & 0xFF), PixelToRgba8(im, o[0].y, o[1].y, o[2].y, (al >> 8) & 0xFF), y - k.band_y0);
    }
  }
}

// What both pair kernels derive from the lane's first column X: the pair it loads, its sigma cell, alpha pair and output offsets
__device__ __forceinline__ void SetPairColumns(PairConst& k, int X) {
  k.outside = X < 0 || X >= k.w;
  // the pair this lane loads: itself, or the pair it mirrors.  One reflection is exact only because the host gate (`even`, decoder.cc)
  // admits w >= 8: the lanes whose pairs reach a stored pixel have X in [-4, w + 2] (second iteration: [-2, w]); lanes further right are
  // clamped and store nothing
  const int xm = X < 0 ? -X - 2 : (X >= k.w ? 2 * k.w - 2 - X : X);
  k.in_bytes = (uint32_t)min(max(xm, 0), k.w - 2) * 4u;
  const int xc = min(max(X, 0), k.w - 2);
  k.cell_bytes = (uint32_t)(xc >> 3) * 4u;
  k.alpha_bytes = (uint32_t)xc;
  k.out_bytes = (uint32_t)xc * 4u;
  k.xb_lo = (X & 7) == 0; k.xb_hi = (X & 7) == 6;   // component 0 is column 0 of a block / component 1 is column 7
}

__global__ __launch_bounds__(256, 4) void filter_stream_pairs_kernel(const DevImage* __restrict__ imgs) {
  JXL_PIXEL_PRIO();
  const DevImage& im = imgs[blockIdx.y];
  if (!im.fused_gab_epf1 || !(im.stream_pairs & 1)) return;
  PairConst k;
  k.w = im.w; k.h = im.h; k.wp = im.wp; k.w8 = im.w8; k.band_y0 = im.band_y0;
  k.to_float = im.fused_gab_epf1 == 2;
  const int band_lo = k.to_float ? max(0, im.band_y0 - 1) : im.band_y0, band_hi = k.to_float ? min(k.h, im.band_y1 + 1) : im.band_y1;
  // (the wavefront's index, given to the compiler as the uniform value it is: rows, segment bounds and row offsets are scalar)
  StripTask t;
  if (!GetStripTask(__builtin_amdgcn_readfirstlane(threadIdx.x / kStripLanes), k.w, band_lo, band_hi, kPairOut, 2, 2, t)) return;
  k.y0 = t.y0; k.y1 = t.y1;
  k.r_end = k.y1 + 3;
  SetPairColumns(k, t.X);   // strips start on multiples of 8
  k.stores = t.stores;
  k.use_alpha = im.has_alpha && !k.to_float;
  k.bpp = im.nch_out;
  k.in0 = PlaneResource(im.stream_in[0]); k.in1 = PlaneResource(im.stream_in[1]); k.in2 = PlaneResource(im.stream_in[2]);
  k.sigma = PlaneResource(im.inv_sigma);
  k.alpha = k.use_alpha ? PlaneResource(im.alpha) : k.in0;   // (ignored without alpha: any readable bytes)
  k.out = PlaneResource(im.out);
  k.f0 = PlaneResource(im.stream_mid[0]); k.f1 = PlaneResource(im.stream_mid[1]); k.f2 = PlaneResource(im.stream_mid[2]);
  FillRowConst(im, k);
  PairState st;
  ZeroWindows(st);
  const int r0 = k.y0 - 3;
  PairRow next = LoadPairRow(k, r0);
  PairAux next_aux = LoadPairAux(k, r0 - 3);
  for (int r = r0; r < k.r_end; r += 4) {   // four rows per trip, unconditionally (see filter_stream_kernel)
    PairStreamRow<0>(im, k, st, next, next_aux, r);
    PairStreamRow<1>(im, k, st, next, next_aux, r + 1);
    PairStreamRow<2>(im, k, st, next, next_aux, r + 2);
    PairStreamRow<3>(im, k, st, next, next_aux, r + 3);
  }
}

// The second EPF iteration (frames with two: distance 1.5 ... 4) + XYB -> output samples, register streaming like the kernel above
// but much lighter: three rows of the first iteration's output (f32 planes), four neighbours, a one-pixel SAD.  Same strip geometry
// (a wavefront = 256 columns, the outer quads are halo), same output paths.  With it a two-iteration frame runs
// reconstruction -> two streaming kernels instead of three LDS-tiled stage kernels (measured, 384 4K frames at distance 2:
// filters + output 104.8 ms before).
__global__ __launch_bounds__(256) void filter_stream2_kernel(const DevImage* __restrict__ imgs) {
  JXL_PIXEL_PRIO();
  const DevImage& im = imgs[blockIdx.y];
  if (im.fused_gab_epf1 != 2 || (im.stream_pairs & 2)) return;   // (RGBA8 frames of even width: filter_stream2_pairs_kernel)
  const int w = im.w, h = im.h, wp = im.wp;
  StripTask t;
  if (!GetStripTask(threadIdx.x / kStripLanes, w, im.band_y0, im.band_y1, kStripOut, 1, 4, t)) return;
  const int q = t.q, X = t.X, y0 = t.y0, y1 = t.y1;
  const bool interior = X >= 0 && X + 3 < w;
  const bool plain = PlainOutput(im);
  const bool fast = plain && im.nch_out == 4 && X + 3 < w;   // whole RGBA quads of the plain layouts
  const JXL_GLOBAL float* in0 = (const JXL_GLOBAL float*)im.stream_mid[0];
  const JXL_GLOBAL float* in1 = (const JXL_GLOBAL float*)im.stream_mid[1];
  const JXL_GLOBAL float* in2 = (const JXL_GLOBAL float*)im.stream_mid[2];
  const JXL_GLOBAL float* inv_sigma = (const JXL_GLOBAL float*)im.inv_sigma;
  const float cs[3] = {im.epf_channel_scale[0], im.epf_channel_scale[1], im.epf_channel_scale[2]};
  const float sm = im.epf_pass2_sigma_scale, smb = sm * im.epf_border_sad_mul;
  const bool xb0 = (q & 1) != 0, xb3 = (q & 1) == 0;
  const int cellx = min(max(X, 0), w - 1) >> 3;
  const int xa = min(max(X, 0), max(w - 4, 0));
  Row3 prev = LoadRow3(in0, in1, in2, X, y0 - 1, w, h, wp, interior);
  Row3 cur = LoadRow3(in0, in1, in2, X, y0, w, h, wp, interior);
  for (int y = y0; y < y1; y++) {
    const Row3 next = LoadRow3(in0, in1, in2, X, y + 1, w, h, wp, interior);
    const float is = inv_sigma[(size_t)(y >> 3) * im.w8 + cellx];
    uint32_t al = 0xFFFFFFFFu;
    if (im.has_alpha && plain) al = LoadAlphaQuad((const JXL_GLOBAL uint8_t*)im.alpha + (size_t)y * w + xa);
    F4 o[3];
    Epf2Row(prev, cur, next, cs, sm, smb, is, y, xb0, xb3, o);
    if (t.stores) StoreQuad(im, o, al, X, y, w, fast);
    prev = cur;
    cur = next;
  }
}

// The second iteration in the two-pixels-per-lane form (RGBA8 + alpha frames of even width): same addressing and edge handling as
// filter_stream_pairs_kernel, one halo pair each side (the iteration reaches one column): 124 output columns per strip.
constexpr int kPair2Out = 2 * (kStripLanes - 2);
__global__ __launch_bounds__(256, 4) void filter_stream2_pairs_kernel(const DevImage* __restrict__ imgs) {
  JXL_PIXEL_PRIO();
  const DevImage& im = imgs[blockIdx.y];
  if (im.fused_gab_epf1 != 2 || !(im.stream_pairs & 2)) return;
  PairConst k;
  k.w = im.w; k.h = im.h; k.wp = im.wp; k.w8 = im.w8; k.band_y0 = im.band_y0;
  StripTask t;
  if (!GetStripTask(__builtin_amdgcn_readfirstlane(threadIdx.x / kStripLanes), k.w, im.band_y0, im.band_y1, kPair2Out, 1, 2, t)) return;
  k.y0 = t.y0; k.y1 = t.y1;
  k.r_end = k.y1 + 1;                               // last input row + 1
  SetPairColumns(k, t.X);                           // strips start on multiples of 4
  k.stores = t.stores;
  k.use_alpha = im.has_alpha != 0;
  k.bpp = im.nch_out;
  k.in0 = PlaneResource(im.stream_mid[0]); k.in1 = PlaneResource(im.stream_mid[1]); k.in2 = PlaneResource(im.stream_mid[2]);
  k.sigma = PlaneResource(im.inv_sigma);
  k.alpha = k.use_alpha ? PlaneResource(im.alpha) : k.in0;
  k.out = PlaneResource(im.out);
  const float cs[3] = {im.epf_channel_scale[0], im.epf_channel_scale[1], im.epf_channel_scale[2]};
  const float sm = im.epf_pass2_sigma_scale, smb = sm * im.epf_border_sad_mul;
  PairRow prev = LoadPairRow(k, k.y0 - 1);
  PairRow cur = LoadPairRow(k, k.y0);
  PairRow next = LoadPairRow(k, min(k.y0 + 1, k.r_end - 1));
  PairAux aux = LoadPairAux(k, k.y0);
  for (int y = k.y0; y < k.y1; y++) {
    // two rows ahead for the pairs, one for sigma / alpha: nothing this row uses was requested in it
    const PairRow next2 = LoadPairRow(k, min(y + 2, k.r_end - 1));
    const PairAux aux2 = LoadPairAux(k, y + 1);
    const uint32_t al = k.use_alpha ? aux.al : 0xFFFFu;
    F2 o[3];
    Epf2Row(prev, cur, next, cs, sm, smb, aux.is, y, k.xb_lo, k.xb_hi, o);
    if (k.stores) {
      StorePixelPair(k, PixelToRgba8(im, o[0].x, o[1].x, o[2].x, al & 0xFF), PixelToRgba8(im, o[0].y, o[1].y, o[2].y, (al >> 8) & 0xFF), y - k.band_y0);
    }
    prev = cur; cur = next; next = next2; aux = aux2;
  }
}

// no loop filter at all: plain conversion
__global__ void out_only_kernel(const DevImage* __restrict__ imgs) {
  const DevImage& im = imgs[blockIdx.y];
  if (im.final_stage != 4) return;
  const int w = im.w, wp = im.wp;
  const size_t n = (size_t)w * (im.band_y1 - im.band_y0);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % w), y = im.band_y0 + (int)(i / w);
    const size_t o = (size_t)y * wp + x;
    WritePixel(im, x, y, im.stage_in[4][0][o], im.stage_in[4][1][o], im.stage_in[4][2][o]);
  }
}

// Reduced-size decode (DevImage::ds): output pixel (cx, cy) is the LF sample of cell (cx, cy) - lf_final after
// dequantisation and adaptive smoothing - through the conversions of the full decode: PixelToRgba8 for the plain 8-bit layouts,
// WritePixelAt for everything else.  No Gaborish, EPF or noise.  Alpha: the cell means alpha_reduce_kernel left in ds_alpha.
// The planes and the output have tight rows, so an un-oriented image is one run of ds_w * ds_h pixels: plain RGBA / RGB output takes
// four pixels per lane (three 16-byte loads, one 16- or 12-byte store; a wavefront stores 1 KiB / 768 B without a gap), the tail of up
// to three pixels and every other layout or orientation one pixel per lane, stored at its oriented position.
__device__ __forceinline__ void LfOutputPixel(const DevImage& im, size_t i, float X, float Y, float B) {
  const int cx = (int)(i % (size_t)im.ds_w), cy = (int)(i / (size_t)im.ds_w);
  const size_t o = OrientedIndex(im.ds_orient, cx, cy, im.ds_w, im.ds_h);
  const uint32_t a = !im.has_alpha ? 0u : (im.out_bits == 8 ? (uint32_t)im.ds_alpha[i] : (im.out_bits == 16 ? (uint32_t)((const uint16_t*)im.ds_alpha)[i]
                                                                                                              : ((const uint32_t*)im.ds_alpha)[i]));
  if (PlainOutput(im)) {
    const uint32_t px = PixelToRgba8(im, X, Y, B, a);
    uint8_t* out = im.out + o * im.nch_out;
    if (im.nch_out == 4) *(uint32_t*)out = px;
    else if (im.nch_out == 3) { out[0] = (uint8_t)px; out[1] = (uint8_t)(px >> 8); out[2] = (uint8_t)(px >> 16); }
    else { out[0] = (uint8_t)(px >> 8); if (im.nch_out == 2) out[1] = (uint8_t)(px >> 24); }
    return;
  }
  WritePixelAt(im, [&] { return o; }, X, Y, B, a);
}
__global__ __launch_bounds__(256) void lf_output_kernel(const DevImage* __restrict__ imgs) {
  const DevImage& im = imgs[blockIdx.y];
  if (!im.ds || im.is_modular) return;
  const size_t n = (size_t)im.ds_w * im.ds_h;
  const float* __restrict__ pX = im.lf_final[0];
  const float* __restrict__ pY = im.lf_final[1];
  const float* __restrict__ pB = im.lf_final[2];
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  const bool quads = PlainOutput(im) && im.ds_orient == 1 && im.ncolor == 3 && ((uintptr_t)im.out & 15) == 0;
  if (!quads) {
    for (size_t i = gid; i < n; i += stride) LfOutputPixel(im, i, pX[i], pY[i], pB[i]);
    return;
  }
  const size_t nq = n >> 2;
  for (size_t q = gid; q < nq; q += stride) {
    const float4 X = ((const float4*)pX)[q], Y = ((const float4*)pY)[q], B = ((const float4*)pB)[q];
    const uint32_t a = im.has_alpha ? ((const uint32_t*)im.ds_alpha)[q] : 0u;
    const uint32_t p0 = PixelToRgba8(im, X.x, Y.x, B.x, a & 0xFF), p1 = PixelToRgba8(im, X.y, Y.y, B.y, (a >> 8) & 0xFF);
    const uint32_t p2 = PixelToRgba8(im, X.z, Y.z, B.z, (a >> 16) & 0xFF), p3 = PixelToRgba8(im, X.w, Y.w, B.w, a >> 24);
    if (im.nch_out == 4) ((uint4*)im.out)[q] = make_uint4(p0, p1, p2, p3);
    else ((uint3*)im.out)[q] = make_uint3((p0 & 0xFFFFFFu) | (p1 << 24), ((p1 >> 8) & 0xFFFFu) | (p2 << 16), ((p2 >> 16) & 0xFFu) | (p3 << 8));
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const size_t i = 4 * nq + threadIdx.x;
    LfOutputPixel(im, i, pX[i], pY[i], pB[i]);
  }
}

void LaunchLfOutput(const DevImage* imgs, int nimg, size_t max_cells, hipStream_t s) {
  if (nimg <= 0) return;
  const size_t b = std::min<size_t>((max_cells + 255) / 256, 2048);
  hipLaunchKernelGGL(lf_output_kernel, dim3((unsigned)std::max<size_t>(1, b), nimg), dim3(256), 0, s, imgs);
}

void LaunchReconTiles(const DevImage* imgs, int nimg, int max_tiles, const float* basis_all, const float* basis_small,
                      const float* llf_scale, const float* basis_mfma, hipStream_t s) {
  const size_t lds = ReconTileLds().end;
  static bool raised = false;
  if (!raised) { (void)hipFuncSetAttribute((const void*)recon_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); raised = true; }
  hipLaunchKernelGGL(recon_tile_kernel, dim3(max_tiles, nimg), dim3(768), lds, s, imgs, basis_all, basis_small, llf_scale, basis_mfma);
}

void LaunchFilterTiles(const DevImage* imgs, int nimg, int max_w, int max_h, int stage_mask, bool any_unfiltered,
                       int any_fused, int any_fused2, hipStream_t s) {   // any_fused / any_fused2: 1 = frames of the pair kernels, 2 = others
  const int tiles = ((max_w + 63) / 64) * ((max_h + 31) / 32);
  dim3 g(tiles, nimg);
  // Gaborish / iteration 0 as stage kernels: frames without EPF, frames with three iterations (before their streaming kernels), taps
  if (stage_mask & 1) hipLaunchKernelGGL(filter_tile_kernel<0>, g, dim3(256), 0, s, imgs);
  if (stage_mask & 2) hipLaunchKernelGGL(filter_tile_kernel<1>, g, dim3(256), 0, s, imgs);
  if (any_fused) {
    // one wavefront per (strip, segment); + 2 rows: the first of two streaming kernels also writes the rows its second one reads
    const int groups = ((max_w + kStripOut - 1) / kStripOut) * ((max_h + 2 + kSegRows - 1) / kSegRows);
    const int pair_groups = ((max_w + kPairOut - 1) / kPairOut) * ((max_h + 2 + kSegRows - 1) / kSegRows);
    if (any_fused & 1) hipLaunchKernelGGL(filter_stream_pairs_kernel, dim3((pair_groups + kGroupsPerWg - 1) / kGroupsPerWg, nimg), dim3(256), 0, s, imgs);
    if (any_fused & 2) hipLaunchKernelGGL(filter_stream_kernel, dim3((groups + kGroupsPerWg - 1) / kGroupsPerWg, nimg), dim3(256), 0, s, imgs);
    const int pair2_groups = ((max_w + kPair2Out - 1) / kPair2Out) * ((max_h + kSegRows - 1) / kSegRows);
    if (any_fused2 & 1) hipLaunchKernelGGL(filter_stream2_pairs_kernel, dim3((pair2_groups + kGroupsPerWg - 1) / kGroupsPerWg, nimg), dim3(256), 0, s, imgs);
    if (any_fused2 & 2) hipLaunchKernelGGL(filter_stream2_kernel, dim3((groups + kGroupsPerWg - 1) / kGroupsPerWg, nimg), dim3(256), 0, s, imgs);
  }
  if (stage_mask & 4) hipLaunchKernelGGL(filter_tile_kernel<2>, g, dim3(256), 0, s, imgs);   // (only with the stage taps)
  if (stage_mask & 8) hipLaunchKernelGGL(filter_tile_kernel<3>, g, dim3(256), 0, s, imgs);
  if (any_unfiltered) {
    size_t work = (size_t)max_w * max_h;
    size_t b = std::min<size_t>((work + 255) / 256, 8192);
    hipLaunchKernelGGL(out_only_kernel, dim3((unsigned)b, nimg), dim3(256), 0, s, imgs);
  }
}

}  // namespace jxlhip
