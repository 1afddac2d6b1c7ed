// HIP kernels (gfx950) of the searched lossless stream, efforts 8 and 9 of SaveImage(lossless) (DESIGN.md §2 "Lossless efforts 8 and
// 9", §4.11).  Efforts up to 7 never launch any of them (encode_kernels.hip: enc_ll_planes_kernel, enc_ll_tokens_kernel).
//
//   enc_ll_count_kernel     the distinct pixels over the coded channels: a hash set in global memory, vector atomics     (scatter)
//   enc_ll_index_kernel     pixels -> palette indices through that set
//   enc_ll_search_kernel    token histograms of the residuals of every (candidate plane, predictor 1..5), one pass        (LDS histograms)
//   enc_ll_planes2_kernel   BGRA8 -> integer planes under the chosen reversible colour transform
//   enc_ll_wp_kernel        forward weighted predictor: prediction + property 15 of every sample, one wavefront per (group, channel),
//                           rows skewed over the lanes                                                                  (register pipeline)
//   enc_ll_tokens2_kernel   tokens + per-leaf histograms under the chosen predictors and (effort 9) property-15 contexts
// Predictors, neighbourhood and the weighted predictor's arithmetic are the decoder's own: modular_rules.h (through enc_dev.h).
#include <hip/hip_runtime.h>
#include "dev_util.h"
#include "enc_dev.h"
#include "enc_types.h"
#include "kernels.h"

namespace jxlhip {

namespace {

// the thresholds of property 15 (the weighted predictor's largest neighbouring error): bucket = how many of them the property exceeds
__device__ const int32_t kWpCuts[kWpLeaves - 1] = {-80, -24, -8, -3, -1, 0, 2, 7, 23, 79};

// key of the pixel over the coded channels, channel k in byte k: Gray(A) takes B (as enc_ll_planes_kernel), RGB(A) is R, G, B(, A)
__device__ __forceinline__ uint32_t PixelKey(const EncImage& im, uchar4 p) {
  uint32_t key = im.gray ? p.x : ((uint32_t)p.z | (uint32_t)p.y << 8 | (uint32_t)p.x << 16);
  if (im.has_alpha) key |= (uint32_t)p.w << (im.gray ? 8 : 24);
  return key;
}
__device__ __forceinline__ uint32_t KeyHash(uint32_t key) { return (key * 0x9E3779B1u) >> 20; }   // 12 bits: kPalSlots
static_assert(kPalSlots == 1u << 12, "KeyHash gives 12 bits");

__device__ __forceinline__ uchar4 LoadPixel(const EncImage& im, int x, int y) {
  return *(const uchar4*)(im.bgra + (size_t)y * im.stride + (size_t)x * 4);
}

// forward reversible colour transform `type` (0..6, permutation 0) of one pixel
__device__ __forceinline__ void ForwardRct(int type, int32_t R, int32_t G, int32_t B, int32_t* out) {
  if (type == 6) {
    const int32_t co = R - B, tmp = B + (co >> 1), cg = G - tmp;
    out[0] = tmp + (cg >> 1); out[1] = co; out[2] = cg;
    return;
  }
  const int second = type >> 1;
  out[0] = R;
  out[1] = second == 1 ? G - R : (second == 2 ? G - ((R + B) >> 1) : G);
  out[2] = (type & 1) ? B - R : B;
}

// the candidate planes of one pixel (enc_types.h: kLlSlots)
__device__ __forceinline__ void Candidates(uchar4 p, int32_t* v) {
  const int32_t R = p.z, G = p.y, B = p.x;
  v[0] = R; v[1] = G; v[2] = G - R; v[3] = G - ((R + B) >> 1); v[4] = B; v[5] = B - R;
  const int32_t co = R - B, tmp = B + (co >> 1), cg = G - tmp;
  v[6] = tmp + (cg >> 1); v[7] = co; v[8] = cg;
  v[9] = p.w;
}

// Value of `v` in the lane below (lane - 1) by a DPP wave shift: one VALU move, no LDS traffic (lane 0 reads 0)
__device__ __forceinline__ int32_t LaneAbove(int32_t v) { return __builtin_amdgcn_update_dpp(0, v, 0x138 /* wave_shr:1 */, 0xF, 0xF, false); }

}  // namespace

// ------------------------------------------------------------------ palette
// Every pixel's key goes into an open-addressing set.  A slot is read first and only an empty one takes an atomic, so a picture of few
// colours costs a load per pixel once its colours are in.  More than kPalCap colours (or a full set, which threads that inserted at
// the same time can cause) raise the flag, and every thread leaves at its next pixel.
__global__ void enc_ll_count_kernel(EncImage im, LlSearch ls) {
  const size_t n = (size_t)im.w * im.h;
  volatile uint32_t* flag = ls.pal_count + 1;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    if (*flag) return;
    const uint64_t want = 1ull << 32 | PixelKey(im, LoadPixel(im, (int)(i % im.w), (int)(i / im.w)));
    uint32_t h = KeyHash((uint32_t)want);
    uint32_t probes = 0;
    for (; probes < kPalSlots; probes++, h = (h + 1) & (kPalSlots - 1)) {
      unsigned long long have = *(volatile unsigned long long*)&ls.pal_set[h];
      if (have == 0) {
        have = atomicCAS(&ls.pal_set[h], 0ull, (unsigned long long)want);
        if (have == 0) {
          if (atomicAdd(ls.pal_count, 1u) + 1 > kPalCap) *flag = 1;
          break;
        }
      }
      if (have == want) break;
    }
    if (probes == kPalSlots) *flag = 1;
  }
}

// ll_plane[0] = index of every pixel in the sorted palette (every colour is in the set: the probe ends at its slot)
__global__ void enc_ll_index_kernel(EncImage im, LlSearch ls) {
  const size_t n = (size_t)im.w * im.h;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const uint64_t want = 1ull << 32 | PixelKey(im, LoadPixel(im, (int)(i % im.w), (int)(i / im.w)));
    uint32_t h = KeyHash((uint32_t)want);
    for (uint32_t probes = 0; probes < kPalSlots && ls.pal_set[h] != want; probes++) h = (h + 1) & (kPalSlots - 1);
    im.ll_plane[0][i] = ls.pal_index[h];
  }
}

// ------------------------------------------------------------------ transform and predictor search
// One pass: every sample's residual under each of the five predictors, for each candidate plane, counted by hybrid-uint token in LDS.
// The host prices a histogram as its zero-order entropy plus the tokens' extra bits (a function of the token), sums the planes of a
// transform, and picks.  Neighbours follow the group's edges, as the coded channels will.
__global__ __launch_bounds__(256) void enc_ll_search_kernel(EncImage im, LlSearch ls) {
  __shared__ uint32_t s_h[kLlSlots * kLlPreds * kEncSyms];
  for (int i = threadIdx.x; i < kLlSlots * kLlPreds * (int)kEncSyms; i += 256) s_h[i] = 0;
  __syncthreads();
  const int g = blockIdx.y;
  const int gx = g % im.xg, gy = g / im.xg;
  const int x0 = gx * kGroupDim, y0 = gy * kGroupDim;
  const int gw = min(kGroupDim, im.w - x0), gh = min(kGroupDim, im.h - y0);
  const int nslots = ls.from_planes ? im.ll_nch : kLlSlots;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < gw * gh; i += gridDim.x * 256) {
    const int y = i / gw, x = i % gw;
    // positions of W, N, NW; (-1, .) stands for the 0 left of the group's first sample
    const int wx = x ? x - 1 : (y ? 0 : -1), wy = x ? y : y - 1;
    const int nx = y ? x : wx, ny = y ? y - 1 : wy;
    const int qx = x && y ? x - 1 : wx, qy = x && y ? y - 1 : wy;
    int32_t v[kLlSlots], W[kLlSlots], N[kLlSlots], NW[kLlSlots];
    if (ls.from_planes) {
#pragma unroll
      for (int c = 0; c < 4; c++) {
        if (c >= im.ll_nch) break;
        const int32_t* pl = im.ll_plane[c] + (size_t)y0 * im.w + x0;
        v[c] = pl[(size_t)y * im.w + x];
        W[c] = wx < 0 ? 0 : pl[(size_t)wy * im.w + wx];
        N[c] = nx < 0 ? 0 : pl[(size_t)ny * im.w + nx];
        NW[c] = qx < 0 ? 0 : pl[(size_t)qy * im.w + qx];
      }
    } else {
      Candidates(LoadPixel(im, x0 + x, y0 + y), v);
      if (wx < 0) {
#pragma unroll
        for (int k = 0; k < kLlSlots; k++) W[k] = 0;
      } else {
        Candidates(LoadPixel(im, x0 + wx, y0 + wy), W);
      }
      if (nx < 0) {
#pragma unroll
        for (int k = 0; k < kLlSlots; k++) N[k] = 0;
      } else {
        Candidates(LoadPixel(im, x0 + nx, y0 + ny), N);
      }
      if (qx < 0) {
#pragma unroll
        for (int k = 0; k < kLlSlots; k++) NW[k] = 0;
      } else {
        Candidates(LoadPixel(im, x0 + qx, y0 + qy), NW);
      }
    }
#pragma unroll
    for (int k = 0; k < kLlSlots; k++) {
      if (k >= nslots || (k == kLlSlots - 1 && !ls.from_planes && !im.has_alpha)) continue;
#pragma unroll
      for (int p = 1; p <= kLlPreds; p++) {
        uint32_t tok, nb, bits;
        HybridD(PackSigned(v[k] - ModularPredictWNNW(p, W[k], N[k], NW[k])), &tok, &nb, &bits);
        atomicAdd(&s_h[(k * kLlPreds + p - 1) * kEncSyms + tok], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kLlSlots * kLlPreds * (int)kEncSyms; i += 256)
    if (s_h[i]) atomicAdd(&ls.hist_search[i], s_h[i]);
}

// BGRA8 -> integer planes under reversible colour transform ls.rct_type (RGB) or as they are (Gray); alpha is the last channel
__global__ void enc_ll_planes2_kernel(EncImage im, LlSearch ls) {
  const size_t n = (size_t)im.w * im.h;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const uchar4 p = LoadPixel(im, (int)(i % im.w), (int)(i / im.w));
    int c = 0;
    if (im.gray) im.ll_plane[c++][i] = p.x;
    else {
      int32_t t[3];
      ForwardRct(ls.rct_type, p.z, p.y, p.x, t);
      im.ll_plane[0][i] = t[0]; im.ll_plane[1][i] = t[1]; im.ll_plane[2][i] = t[2];
      c = 3;
    }
    if (im.has_alpha) im.ll_plane[c][i] = p.w;
  }
}

// ------------------------------------------------------------------ forward weighted predictor
// One wavefront per (group, channel).  The encoder knows every sample, so the only recurrence is the predictor's error state: a
// sample needs the true error and the four sub-predictor errors of columns x-1 .. x+1 of the row above, and of x-1 (and, through
// the format's "+=" into the row above, x-2) of its own row.  Rows run skewed: lane l holds row r0 + l and works on column
// t - 2l at step t, so the lane above finished column x+1 one step earlier and hands its five values down by a wave shift; N and NW
// are what came down one and two steps before.  The own row's state stays in registers.  A 256-row group is four 64-row bands; the
// last row of a band reaches the next band's lane 0 through one LDS row of 5 * (w + 2) words.  Bit-identical to the decoder's
// WpState (modular_rules.h: WpPredictFromState, written out here once more with that header's WpErrorWeight / WpAbs - through the shared
// function this kernel took two more registers), edge clamps and carry included: tests/test_gpu_lossless_effort.py round-trips through it.
__global__ __launch_bounds__(64) void enc_ll_wp_kernel(EncImage im, LlSearch ls) {
  __shared__ int32_t s_row[5][kGroupDim + 2];
  __shared__ uint32_t s_h[kEncSyms];
  const int lane = threadIdx.x;
  const int g = blockIdx.x / im.ll_nch, c = blockIdx.x % im.ll_nch;
  const int gx = g % im.xg, gy = g / im.xg;
  const int x0 = gx * kGroupDim, y0 = gy * kGroupDim;
  const int gw = min(kGroupDim, im.w - x0), gh = min(kGroupDim, im.h - y0);
  const size_t origin = (size_t)y0 * im.w + x0;
  const int32_t* pl = im.ll_plane[c] + origin;
  int32_t* out_pred = ls.wp_pred[c] + origin;
  int32_t* out_prop = ls.wp_prop[c] + origin;
  for (int i = lane; i < (int)kEncSyms; i += 64) s_h[i] = 0;
  for (int b0 = 0; b0 < gh; b0 += 64) {
    // the band before has written its last row (LDS operations of one wavefront execute in order; this holds the compiler to it)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int rows = min(64, gh - b0);
    const int y = b0 + lane;
    const bool row_on = lane < rows;
    const bool hand_on = lane == 63 && b0 + 64 < gh;   // this row is the next band's row above
    const int32_t* cur = pl + (size_t)(row_on ? y : 0) * im.w;
    // row above, columns x-1, x, x+1: true error and sub-predictor errors as that row stored them
    int32_t a_err[3] = {0, 0, 0};
    uint32_t a_e[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    // own row: true error of x-1, sub-predictor errors of x-1 and x-2, the sample at x-1
    int32_t o_err = 0, W = 0;
    uint32_t o_e1[4] = {0, 0, 0, 0}, o_e2[4] = {0, 0, 0, 0};
    if (lane == 0 && b0 > 0) {   // lane 0 starts at column 0 with no steps before it: column 0 of the row above is already due
      a_err[2] = s_row[0][0];
#pragma unroll
      for (int i = 0; i < 4; i++) a_e[i][2] = (uint32_t)s_row[1 + i][0];
    }
    const int steps = gw + 2 * (rows - 1);
    for (int t = 0; t < steps; t++) {
      const int x = t - 2 * lane;
      // column x+1 of the row above: the lane above finished it in the step before
      int32_t up_err = LaneAbove(o_err);
      uint32_t up_e[4];
#pragma unroll
      for (int i = 0; i < 4; i++) up_e[i] = (uint32_t)LaneAbove((int32_t)o_e1[i]);
      if (lane == 0) {
        const bool have = b0 > 0 && x + 1 < gw;
        up_err = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) up_e[i] = 0;
        if (have) {
          up_err = s_row[0][x + 1];
#pragma unroll
          for (int i = 0; i < 4; i++) up_e[i] = (uint32_t)s_row[1 + i][x + 1];
        }
      }
      a_err[0] = a_err[1]; a_err[1] = a_err[2]; a_err[2] = up_err;
#pragma unroll
      for (int i = 0; i < 4; i++) { a_e[i][0] = a_e[i][1]; a_e[i][1] = a_e[i][2]; a_e[i][2] = up_e[i]; }
      if (!row_on || x < 0 || x >= gw) continue;
      // the sample's neighbourhood, as the decoder's ModularChannel sees it
      const int32_t v = cur[x];
      if (x == 0) W = y ? cur[-(ptrdiff_t)im.w] : 0;
      const int32_t Np = y ? cur[x - (ptrdiff_t)im.w] : W;
      const int32_t NEp = y && x + 1 < gw ? cur[x + 1 - (ptrdiff_t)im.w] : Np;   // (the default sub-predictors read neither NW nor NN)
      // error state with the format's edge clamps (NE of the last column and NW of the first are N), and the carry: every finished
      // sample of this row has added its sub-predictor errors to the row above at the next column
      const bool first = x == 0, last = x == gw - 1;
      const int64_t teW = first ? 0 : o_err, teN = a_err[1], teNW = first ? a_err[1] : a_err[0], teNE = last ? a_err[1] : a_err[2];
      const uint32_t kW[4] = {13, 12, 12, 12};
      uint32_t weights[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint32_t pN = a_e[i][1] + o_e1[i];
        const uint32_t pNW = first ? pN : a_e[i][0] + o_e2[i];
        const uint32_t pNE = last ? pN : a_e[i][2];
        weights[i] = WpErrorWeight((uint64_t)pN + pNE + pNW, kW[i], WpDivExact());
      }
      const int64_t N8 = (int64_t)Np << 3, W8 = (int64_t)W << 3, NE8 = (int64_t)NEp << 3;
      const int64_t sumWN = teN + teW;
      int64_t p = teW;
      if (WpAbs(teN) > WpAbs(p)) p = teN;
      if (WpAbs(teNW) > WpAbs(p)) p = teNW;
      if (WpAbs(teNE) > WpAbs(p)) p = teNE;
      int64_t prediction[4];
      prediction[0] = W8 + NE8 - N8;
      prediction[1] = N8 - (((sumWN + teNE) * 16) >> 5);
      prediction[2] = W8 - (((sumWN + teNW) * 10) >> 5);
      prediction[3] = N8 - ((teNW * 7 + teN * 7 + teNE * 7) >> 5);
      uint32_t weight_sum = weights[0] + weights[1] + weights[2] + weights[3];
      const int log_weight = 31 - __clz(weight_sum);
      weight_sum = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) { weights[i] >>= log_weight - 4; weight_sum += weights[i]; }
      int64_t sum = (int64_t)(weight_sum >> 1) - 1;
#pragma unroll
      for (int i = 0; i < 4; i++) sum += prediction[i] * (int64_t)weights[i];
      int64_t pred = (sum * (int64_t)WpDivExact()(weight_sum - 1)) >> 24;
      if (((teN ^ teW) | (teN ^ teNW)) <= 0) {
        const int64_t mx = W8 > NE8 ? (W8 > N8 ? W8 : N8) : (NE8 > N8 ? NE8 : N8), mn = W8 < NE8 ? (W8 < N8 ? W8 : N8) : (NE8 < N8 ? NE8 : N8);
        pred = pred < mn ? mn : (pred > mx ? mx : pred);
      }
      const int32_t guess = (int32_t)((pred + 3) >> 3);
      out_pred[(size_t)y * im.w + x] = guess;
      out_prop[(size_t)y * im.w + x] = (int32_t)p;
      {
        uint32_t tok, nb, bits;
        HybridD(PackSigned(v - guess), &tok, &nb, &bits);
        atomicAdd(&s_h[tok], 1u);
      }
      // the state after this sample
      const int64_t v8 = (int64_t)v << 3;
      o_err = (int32_t)(pred - v8);
#pragma unroll
      for (int i = 0; i < 4; i++) { o_e2[i] = o_e1[i]; o_e1[i] = (uint32_t)((WpAbs(prediction[i] - v8) + 3) >> 3); }
      W = v;
      if (hand_on) {
        s_row[0][x] = o_err;
#pragma unroll
        for (int i = 0; i < 4; i++) s_row[1 + i][x] = (int32_t)o_e1[i];
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  for (int i = lane; i < (int)kEncSyms; i += 64)
    if (s_h[i]) atomicAdd(&ls.hist_wp[c * kEncSyms + i], s_h[i]);
}

// ------------------------------------------------------------------ tokens
// Residuals of every channel of one group under the chosen predictors; the context is the channel's leaf, at effort 9 the leaf of
// the channel's property-15 bucket.  Group 0's tokens start after ll_tok_extra (a palette's colours, put there by the host).
__global__ __launch_bounds__(256) void enc_ll_tokens2_kernel(EncImage im, LlSearch ls) {
  __shared__ uint32_t s_h[kLlMaxLeaves * kEncSyms];
  for (int i = threadIdx.x; i < (int)(kLlMaxLeaves * kEncSyms); i += 256) s_h[i] = 0;
  __syncthreads();
  const int g = blockIdx.y;
  const int gx = g % im.xg, gy = g / im.xg;
  const int x0 = gx * kGroupDim, y0 = gy * kGroupDim;
  const int gw = min(kGroupDim, im.w - x0), gh = min(kGroupDim, im.h - y0);
  const int per = gw * gh, n = per * im.ll_nch;
  const size_t origin = (size_t)y0 * im.w + x0;
  DevToken* out = im.tok_ll + (size_t)g * kLlTokCap + (g ? 0u : im.ll_tok_extra);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int c = i / per, r = i % per, y = r / gw, x = r % gw;
    const int32_t* pl = im.ll_plane[c] + origin;
    const size_t at = (size_t)y * im.w + x;
    const int32_t v = pl[at];
    const int pred = ls.pred[c];
    int32_t guess;
    if (pred == 6) guess = ls.wp_pred[c][origin + at];
    else {
      const ModularWNNW hd = ModularWNNWAt([&](int sx, int sy) { return pl[(size_t)sy * im.w + sx]; }, x, y);
      guess = ModularPredictWNNW(pred, hd.W, hd.N, hd.NW);
    }
    int bucket = 0;
    if (ls.wp_ctx) {
      const int32_t prop = ls.wp_prop[c][origin + at];
#pragma unroll
      for (int k = 0; k < kWpLeaves - 1; k++) bucket += prop > kWpCuts[k];
    }
    DevToken t;
    t.ctx = ls.ctx[c][bucket];
    t.value = PackSigned(v - guess);
    out[i] = t;
    uint32_t tok, nb, bits;
    HybridD(t.value, &tok, &nb, &bits);
    atomicAdd(&s_h[t.ctx * kEncSyms + tok], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < (int)(kLlMaxLeaves * kEncSyms); i += 256)
    if (s_h[i]) atomicAdd(&ls.hist_ll[i], s_h[i]);
}

// ------------------------------------------------------------------ launch wrappers
static inline unsigned GridFor(size_t work, unsigned cap = 8192) {
  size_t b = (work + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// stage 0: colour count; 1: palette indices; 2: search; 3: planes; 4: weighted pass; 5: tokens
void LaunchEncLosslessSearch(const EncImage& im, const LlSearch& ls, int stage, hipStream_t s) {
  const size_t npx = (size_t)im.w * im.h;
  switch (stage) {
    case 0: hipLaunchKernelGGL(enc_ll_count_kernel, dim3(GridFor(npx, 2048)), dim3(256), 0, s, im, ls); break;
    case 1: hipLaunchKernelGGL(enc_ll_index_kernel, dim3(GridFor(npx)), dim3(256), 0, s, im, ls); break;
    case 2: hipLaunchKernelGGL(enc_ll_search_kernel, dim3(32, im.ng), dim3(256), 0, s, im, ls); break;
    case 3: hipLaunchKernelGGL(enc_ll_planes2_kernel, dim3(GridFor(npx)), dim3(256), 0, s, im, ls); break;
    case 4: hipLaunchKernelGGL(enc_ll_wp_kernel, dim3((unsigned)(im.ng * im.ll_nch)), dim3(64), 0, s, im, ls); break;
    default: hipLaunchKernelGGL(enc_ll_tokens2_kernel, dim3(32, im.ng), dim3(256), 0, s, im, ls); break;
  }
}

}  // namespace jxlhip
