// The per-sample rules of the Modular sample path, each stated once for host and device: signed packing, the predictors, the
// properties an MA tree may test, the neighbourhood at the channel's edges and its roll from sample to sample, what a leaf and a token
// say, the walk over the static properties, and the weighted predictor with the format's default parameters.  No kernel, no bit
// reader, no table type: the decoders (entropy_kernels.hip, modular_uniform.h), the lossless encoder (encode_kernels.hip,
// lossless_kernels.hip, encoder.cc) and the self tests (selftest.cc) all call these.  Where a loop keeps its state (registers, lanes,
// LDS or global rows) is that loop's business; what the numbers are is decided here.  The CPU suite checks every function against the
// format's definition written out in Python (tests/test_modular_rules.py, through jxlhip_selftest_modular_*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace jxlhip {

// ------------------------------------------------------------------ signed packing
__host__ __device__ __forceinline__ uint32_t PackSigned(int32_t v) { return v >= 0 ? (uint32_t)v << 1 : (((uint32_t)(-(int64_t)v)) << 1) - 1; }
__host__ __device__ __forceinline__ int32_t UnpackSigned(uint32_t u) { return (int32_t)(u >> 1) ^ -(int32_t)(u & 1); }

// ------------------------------------------------------------------ neighbourhood
// Sample (x, y) of a w x h channel sees W, N, NW, NE, NN, WW, NEE.  Outside the channel: the first sample of a row takes the sample
// above it for W (0 in the top row); in the top row N = W; in the first column NW = W, elsewhere in the top row NW = W too; NE = N in
// the last column (and the top row), NEE = NE in the last two; NN = N in the rows 0 and 1; WW = W in the columns 0 and 1.
__host__ __device__ __forceinline__ bool HasNE(int x, int y, int w) { return y && x + 1 < w; }    // else NE = N
__host__ __device__ __forceinline__ bool HasNEE(int x, int y, int w) { return y && x + 2 < w; }   // else NEE = NE
__host__ __device__ __forceinline__ bool HasNN(int y) { return y > 1; }                           // else NN = N

struct ModularHood {
  int32_t W, N, NW, NE, NN, WW, NEE;
  int64_t prev9;    // W + N - NW of the sample before (0 for a row's first): what property 8 subtracts
  int64_t wp_err;   // property 15: the weighted predictor's largest neighbouring true error
  int x, y;
};

// W, N and NW by position, for code that holds the whole channel and predicts from these three (the encoder): at(x, y) reads a sample.
struct ModularWNNW { int32_t W, N, NW; };
template <class At>
__host__ __device__ __forceinline__ ModularWNNW ModularWNNWAt(At at, int x, int y) {
  ModularWNNW h;
  if (x == 0) {
    h.W = y ? at(0, y - 1) : 0; h.N = h.W; h.NW = h.W;
  } else {
    h.W = at(x - 1, y);
    h.N = y ? at(x, y - 1) : h.W;
    h.NW = y ? at(x - 1, y - 1) : h.W;
  }
  return h;
}

// The same neighbourhood carried along a row: what a decode loop keeps in registers.  StartRow before a row's first sample (`above`:
// sample (0, y - 1), 0 in the top row); Step after every sample with the sample's value and its NE (the N of the next one).  NE, NN and
// NEE come from the row store of the caller (HasNE / HasNN / HasNEE say when).  A loop that learns the next N only later takes the
// step in its two halves: StepW after the sample, StepN when that N has arrived.
struct ModularRoll {
  int32_t W, N, NW, WW;
  int64_t prev9;
  __host__ __device__ __forceinline__ void StartRow(int32_t above) { W = above; N = above; NW = above; WW = above; prev9 = 0; }
  __host__ __device__ __forceinline__ void StepW(int32_t val, int x) {
    prev9 = (int64_t)W + N - NW;
    WW = x >= 1 ? W : val;
    W = val;
  }
  __host__ __device__ __forceinline__ void StepN(int32_t NE, int y) {
    if (y) { NW = N; N = NE; } else { NW = W; N = W; }
  }
  __host__ __device__ __forceinline__ void Step(int32_t val, int32_t NE, int x, int y) { StepW(val, x); StepN(NE, y); }
};

// ------------------------------------------------------------------ predictors 0 .. 13
// In 64-bit arithmetic, as the format has them; a sample takes the low 32 bits of residual + prediction.  kPred is the compile-time id
// of the loops that are specialised for one predictor; ModularPredict takes any.  Divisions truncate toward zero.
template <int kPred>
__host__ __device__ __forceinline__ int64_t ModularPredictT(int32_t W, int32_t N, int32_t NW, int32_t NE, int32_t NN, int32_t WW, int32_t NEE,
                                                            int64_t wp_pred) {
  static_assert(kPred >= 0 && kPred <= 13, "the format has predictors 0 .. 13");
  if constexpr (kPred == 0) return 0;
  else if constexpr (kPred == 1) return W;
  else if constexpr (kPred == 2) return N;
  else if constexpr (kPred == 3) return ((int64_t)W + N) / 2;
  else if constexpr (kPred == 4) {   // Select: the neighbour nearer to W + N - NW
    int64_t pp = (int64_t)W + N - NW, pa = pp - W, pb = pp - N;
    if (pa < 0) pa = -pa;
    if (pb < 0) pb = -pb;
    return pa < pb ? W : N;
  } else if constexpr (kPred == 5) {   // clamped gradient
    const int64_t mn = W < N ? W : N, mx = W < N ? N : W, gr = (int64_t)W + N - NW;
    return gr < mn ? mn : (gr > mx ? mx : gr);
  } else if constexpr (kPred == 6) return wp_pred;
  else if constexpr (kPred == 7) return NE;
  else if constexpr (kPred == 8) return NW;
  else if constexpr (kPred == 9) return WW;
  else if constexpr (kPred == 10) return ((int64_t)W + NW) / 2;
  else if constexpr (kPred == 11) return ((int64_t)NW + N) / 2;
  else if constexpr (kPred == 12) return ((int64_t)N + NE) / 2;
  else return (6 * (int64_t)N - 2 * (int64_t)NN + 7 * (int64_t)W + WW + NEE + 3 * (int64_t)NE + 8) / 16;
}
__host__ __device__ __forceinline__ int64_t ModularPredict(uint32_t pred, int32_t W, int32_t N, int32_t NW, int32_t NE, int32_t NN, int32_t WW,
                                                           int32_t NEE, int64_t wp_pred) {
  switch (pred) {
#define JXL_PRED_CASE(k) case k: return ModularPredictT<k>(W, N, NW, NE, NN, WW, NEE, wp_pred)
    JXL_PRED_CASE(1); JXL_PRED_CASE(2); JXL_PRED_CASE(3); JXL_PRED_CASE(4); JXL_PRED_CASE(5); JXL_PRED_CASE(6); JXL_PRED_CASE(7);
    JXL_PRED_CASE(8); JXL_PRED_CASE(9); JXL_PRED_CASE(10); JXL_PRED_CASE(11); JXL_PRED_CASE(12); JXL_PRED_CASE(13);
#undef JXL_PRED_CASE
    default: return 0;   // predictor 0 (ids the format does not have never reach a decoder: the host refuses the tree)
  }
}
// Predictors 1 .. 5, the ones over W, N and NW that the encoder searches; any other id is the gradient.
__host__ __device__ __forceinline__ int32_t ModularPredictWNNW(uint32_t pred, int32_t W, int32_t N, int32_t NW) {
  switch (pred) {
    case 1: return W;
    case 2: return N;
    case 3: return (int32_t)ModularPredictT<3>(W, N, NW, 0, 0, 0, 0, 0);
    case 4: return (int32_t)ModularPredictT<4>(W, N, NW, 0, 0, 0, 0, 0);
    default: return (int32_t)ModularPredictT<5>(W, N, NW, 0, 0, 0, 0, 0);
  }
}

// Predictor 5 in 32-bit arithmetic: min(W, N) if NW >= max, max if NW <= min, else W + N - NW (inside the interval the sum cannot
// overflow).  The form of the row-parallel loops; equal to ModularPredictT<5> on every input.
__host__ __device__ __forceinline__ int32_t ClampedGradient32(int32_t W, int32_t N, int32_t NW) {
  const int32_t mn = W < N ? W : N, mx = W < N ? N : W;
  return NW >= mx ? mn : (NW <= mn ? mx : (int32_t)((uint32_t)W + (uint32_t)N - (uint32_t)NW));
}
// Predictor 5 as the median of W, N and W + N - NW (the clamp of the sum to [min(W, N), max(W, N)]): three dependent operations where
// the device has a median instruction.  Equal to ClampedGradient32 wherever the sum does not overflow; meant for small samples (the
// u8 rows of the one-pass alpha decode), where it cannot.
__host__ __device__ __forceinline__ int32_t ClampedGradientSmall(int32_t W, int32_t N, int32_t NW) {
  const int32_t s = (int32_t)((uint32_t)W + ((uint32_t)N - (uint32_t)NW));
  const int32_t mn = W < N ? W : N, mx = W < N ? N : W;
  const int32_t lo = mx < s ? mx : s;   // min(max(W, N), s)
  return mn > lo ? mn : lo;             // max(min(W, N), min(max(W, N), s)): the median of the three
}
// Predictors 0, 1, 2 and 5 (the ones a row-static channel may use) without a branch, low 32 bits.
__host__ __device__ __forceinline__ uint32_t RowGuess(uint32_t pred, int32_t W, int32_t N, int32_t NW) {
  const uint32_t g = (uint32_t)ClampedGradient32(W, N, NW);
  return pred == 0 ? 0u : (pred == 1 ? (uint32_t)W : (pred == 2 ? (uint32_t)N : g));
}

// ------------------------------------------------------------------ properties 2 .. 15
// (0 and 1, channel and stream, are static: StaticChild below.)
__host__ __device__ __forceinline__ int64_t ModularProperty(int id, const ModularHood& h) {
  switch (id) {
    case 2: return h.y;
    case 3: return h.x;
    case 4: return h.N < 0 ? -(int64_t)h.N : h.N;
    case 5: return h.W < 0 ? -(int64_t)h.W : h.W;
    case 6: return h.N;
    case 7: return h.W;
    case 8: return (int64_t)h.W - h.prev9;
    case 9: return (int64_t)h.W + h.N - h.NW;
    case 10: return (int64_t)h.W - h.NW;
    case 11: return (int64_t)h.NW - h.N;
    case 12: return (int64_t)h.N - h.NE;
    case 13: return (int64_t)h.N - h.NN;
    case 14: return (int64_t)h.W - h.WW;
    case 15: return h.wp_err;
    default: return 0;
  }
}
// The same properties as data: property = [abs] (cW W + cN N + cNW NW + cNE NE + cNN NN + cWW WW + cX x + cY y + cE wp_err
// - [minus_prev9] prev9).  What the grid of modular_uniform.h evaluates, one property per lane, without a branch on the id.
struct PropertyForm {
  int32_t cW, cN, cNW, cNE, cNN, cWW, cX, cY, cE;
  bool abs, minus_prev9;
};
// Written as comparisons on the id, not as a table: the id is a per-lane value where the grid is set up, and with the coefficients
// visibly -1, 0 or 1 the row loop's products with them compile to selects (a table cost the gradient-context 4K stream 8 % of its time).
__host__ __device__ __forceinline__ PropertyForm ModularPropertyForm(int id) {
  PropertyForm f;
  f.cW = (id == 5 || id == 7 || id == 8 || id == 9 || id == 10 || id == 14) ? 1 : 0;
  f.cN = (id == 4 || id == 6 || id == 9 || id == 12 || id == 13) ? 1 : (id == 11 ? -1 : 0);
  f.cNW = id == 11 ? 1 : ((id == 9 || id == 10) ? -1 : 0);
  f.cNE = id == 12 ? -1 : 0;
  f.cNN = id == 13 ? -1 : 0;
  f.cWW = id == 14 ? -1 : 0;
  f.cX = id == 3 ? 1 : 0;
  f.cY = id == 2 ? 1 : 0;
  f.cE = id == 15 ? 1 : 0;
  f.abs = id == 4 || id == 5;
  f.minus_prev9 = id == 8;
  return f;
}

// ------------------------------------------------------------------ leaf and token
// A leaf node (property < 0) holds predictor | context << 8 in `a`, the multiplier in `b` and the offset in `splitval`.
template <class Node> __host__ __device__ __forceinline__ uint32_t LeafPredictor(const Node& nd) { return nd.a & 0xFF; }
template <class Node> __host__ __device__ __forceinline__ uint32_t LeafContext(const Node& nd) { return nd.a >> 8; }
// residual = UnpackSigned(token value) * multiplier + offset, wrapping: the low 32 bits of the format's 64-bit arithmetic, which is all
// a 32-bit sample keeps of it
__host__ __device__ __forceinline__ uint32_t LeafResidual(uint32_t u, uint32_t mul, uint32_t off) { return (uint32_t)UnpackSigned(u) * mul + off; }
// A cluster's hybrid-integer configuration word: split exponent | msb << 4 | lsb << 8, bit 12 when the cluster's code has one
// symbol (nothing is read for it), then that symbol from bit 16.  A token of such a code costs no bits at all when the symbol is
// below the split (no hybrid tail either): every sample of the context then has the residual of OneSymbol().  The symbol is the whole
// upper half of the word: an ANS symbol is below 256, a prefix code's single symbol may be larger (and is then never below a split).
__host__ __device__ __forceinline__ bool OneSymbolCode(uint32_t cfg) { return (cfg & 0x1000) != 0; }
__host__ __device__ __forceinline__ uint32_t OneSymbol(uint32_t cfg) { return cfg >> 16; }
__host__ __device__ __forceinline__ bool OneSymbolToken(uint32_t cfg) { return OneSymbolCode(cfg) && OneSymbol(cfg) < (1u << (cfg & 0xF)); }

// ------------------------------------------------------------------ static walk
// Properties 0 (channel), 1 (stream) and 2 (row) do not depend on decoded samples.  StaticChild: the child such a node sends
// (chan, sid, y) to.  StaticWalk follows them from node `at` - with kRow the row too, setting *used_y - and returns the index of the
// first node that is a leaf or tests something else, with that node in *out.  node_at(i) reads node i (any address space, any node type
// with the fields of DevTreeNode).
template <class Node>
__host__ __device__ __forceinline__ uint32_t StaticChild(const Node& nd, int chan, int sid, int y) {
  const int v = nd.property == 0 ? chan : (nd.property == 1 ? sid : y);
  return v > nd.splitval ? nd.a : nd.b;
}
template <bool kRow, class NodeAt, class Node>
__host__ __device__ __forceinline__ uint32_t StaticWalk(NodeAt node_at, uint32_t at, int chan, int sid, int y, bool* used_y, Node* out) {
  Node nd = node_at(at);
  while (nd.property >= 0 && nd.property <= (kRow ? 2 : 1)) {
    if (kRow && nd.property == 2) *used_y = true;
    at = StaticChild(nd, chan, sid, y);
    nd = node_at(at);
  }
  *out = nd;
  return at;
}

// ------------------------------------------------------------------ weighted predictor, default parameters
// The format's "self-correcting" predictor: four sub-predictors, each weighted by the inverse of the errors it made around the sample.
// A caller keeps, however it likes, the true error (prediction x 8 - sample x 8) and the four sub-predictor errors of every sample of
// this row and the row above, and hands in for sample (x, y):
//   te[4]    the true errors at W, N, NW, NE (W: 0 in the first column; NW / NE: N's in the first / last column)
//   esum[4]  per sub-predictor, the errors at N + NW + NE with the same edge rule, where every error includes what the format's
//            update adds to the next column of the row above (WpSubError of the sample before, and of the one before that for NW)
// and gets the prediction x 8 (pred8; the predictor-6 guess is WpGuess(pred8)), the sub-predictions x 8 and property 15.
struct WpDivExact {   // Div(i) = 2^24 / (i + 1); a loop that holds the 64 quotients in a table passes its lookup instead
  __host__ __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return (1u << 24) / (i + 1); }
};
template <class Div>
__host__ __device__ __forceinline__ uint32_t WpErrorWeight(uint64_t x, uint32_t maxweight, Div div) {
  int shift = (63 - __builtin_clzll(x + 1)) - 5;
  if (shift < 0) shift = 0;
  return 4 + (uint32_t)((maxweight * (uint64_t)div((uint32_t)(x >> shift))) >> shift);
}
__host__ __device__ __forceinline__ int64_t WpAbs(int64_t v) { return v < 0 ? -v : v; }
struct WpPrediction {
  int64_t pred8;     // the prediction x 8
  int64_t sub[4];    // the sub-predictions x 8
  int64_t max_err;   // property 15: the true error of largest magnitude among W, N, NW, NE (the first of equals)
};
template <class Div>
__host__ __device__ __forceinline__ WpPrediction WpPredictFromState(const int64_t te[4], const uint64_t esum[4], int32_t W_, int32_t N_, int32_t NE_, Div div) {
  const int64_t teW = te[0], teN = te[1], teNW = te[2], teNE = te[3];
  const int64_t W = (int64_t)W_ << 3, N = (int64_t)N_ << 3, NE = (int64_t)NE_ << 3;
  WpPrediction r;
  uint32_t weights[4];
#pragma unroll
  for (int i = 0; i < 4; i++) weights[i] = WpErrorWeight(esum[i], i == 0 ? 13u : 12u, div);
  const int64_t sumWN = teN + teW;
  int64_t p = teW;
  if (WpAbs(teN) > WpAbs(p)) p = teN;
  if (WpAbs(teNW) > WpAbs(p)) p = teNW;
  if (WpAbs(teNE) > WpAbs(p)) p = teNE;
  r.max_err = p;
  r.sub[0] = W + NE - N;
  r.sub[1] = N - (((sumWN + teNE) * 16) >> 5);
  r.sub[2] = W - (((sumWN + teNW) * 10) >> 5);
  r.sub[3] = N - ((teNW * 7 + teN * 7 + teNE * 7) >> 5);
  uint32_t weight_sum = weights[0] + weights[1] + weights[2] + weights[3];
  const int log_weight = 31 - __builtin_clz(weight_sum);
  weight_sum = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) { weights[i] >>= log_weight - 4; weight_sum += weights[i]; }
  int64_t sum = (int64_t)(weight_sum >> 1) - 1;
#pragma unroll
  for (int i = 0; i < 4; i++) sum += r.sub[i] * (int64_t)weights[i];
  int64_t pred = (sum * (int64_t)div(weight_sum - 1)) >> 24;
  if (((teN ^ teW) | (teN ^ teNW)) <= 0) {   // unless the errors at W, N and NW agree in sign: inside the span of W, N, NE
    const int64_t mx = W > NE ? (W > N ? W : N) : (NE > N ? NE : N), mn = W < NE ? (W < N ? W : N) : (NE < N ? NE : N);
    pred = pred < mn ? mn : (pred > mx ? mx : pred);
  }
  r.pred8 = pred;
  return r;
}
__host__ __device__ __forceinline__ int64_t WpGuess(int64_t pred8) { return (pred8 + 3) >> 3; }
// What a decoded sample leaves behind: its true error, and per sub-predictor the error that is stored at its place and added to the next
// column of the row above.
__host__ __device__ __forceinline__ int32_t WpTrueError(int64_t pred8, int64_t val) { return (int32_t)(pred8 - (val << 3)); }
__host__ __device__ __forceinline__ uint32_t WpSubError(int64_t sub, int64_t val) { return (uint32_t)((WpAbs(sub - (val << 3)) + 3) >> 3); }

// The state in its memory form, as the format defines it: the true error and the four sub-predictor errors of the current and the
// previous row, (w + 2) entries each, in a scratch of kInts * (w + 2) words (LDS when it fits, global memory otherwise).
struct WpState {
  static constexpr int kInts = 10;
  int32_t* err;                // [2][w + 2]
  uint32_t* pe;                // [4][2][w + 2]
  int w2;                      // w + 2
  WpPrediction last;
  __host__ __device__ void Init(int32_t* scratch, int w) {
    w2 = w + 2;
    err = scratch;
    pe = (uint32_t*)(err + 2 * w2);
    for (int i = 0; i < kInts * w2; i++) err[i] = 0;
  }
  // the predictor-6 guess of sample (x, y); *max_err: property 15
  __host__ __device__ int64_t Predict(int x, int y, int w, int32_t N, int32_t W, int32_t NE, int64_t* max_err) {
    const int cur = (y & 1) ? 0 : w2, prev = (y & 1) ? w2 : 0;
    const int pN = prev + x, pNE = x < w - 1 ? pN + 1 : pN, pNW = x > 0 ? pN - 1 : pN;
    uint64_t esum[4];
    for (int i = 0; i < 4; i++) {
      const uint32_t* p = pe + (size_t)i * 2 * w2;
      esum[i] = (uint64_t)p[pN] + p[pNE] + p[pNW];
    }
    const int64_t te[4] = {x == 0 ? 0 : err[cur + x - 1], err[pN], err[pNW], err[pNE]};
    last = WpPredictFromState(te, esum, W, N, NE, WpDivExact());
    *max_err = last.max_err;
    return WpGuess(last.pred8);
  }
  __host__ __device__ void Update(int64_t val, int x, int y) {
    const int cur = (y & 1) ? 0 : w2, prev = (y & 1) ? w2 : 0;
    err[cur + x] = WpTrueError(last.pred8, val);
    for (int i = 0; i < 4; i++) {
      const uint32_t e = WpSubError(last.sub[i], val);
      uint32_t* p = pe + (size_t)i * 2 * w2;
      p[cur + x] = e;
      p[prev + x + 1] += e;
    }
  }
};

}  // namespace jxlhip
