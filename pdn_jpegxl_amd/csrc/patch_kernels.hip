// HIP kernel (gfx950) of patches: rectangles of reference-only frames (atlases) blended into a frame's own f32 samples, in place, after
// the frame is decoded and before it is composited onto the canvas (DESIGN.md §2 has the rules, §4.8 the measurements).
//
// One workgroup per 64x64 tile of a patched frame that at least one position touches; tiles without patches have no workgroup.  The
// host lists each tile's positions in dictionary order and the union of their rectangles (the tile's box): only the box is read and
// written.  Four wavefronts, one per row residue: a lane owns one column and the 16 rows of its wavefront, keeps those pixels in
// registers while it walks the tile's positions (descriptors uniform per workgroup: scalar loads), and stores the ones a patch touched.
// Each pixel belongs to one lane, so overlapping positions apply in order with no atomics.  The atlases are other frames of the batch,
// never written here (patches on reference-only frames are refused on the host).
#include <hip/hip_runtime.h>
#include <algorithm>
#include "dev_types.h"
#include "dev_util.h"
#include "kernels.h"

namespace jxlhip {
namespace {

__device__ __forceinline__ float Clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float Lane(float4 v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }

// NCH f32 samples of pixel i: one 16-, 12-, 8- or 4-byte access
template <int NCH>
__device__ __forceinline__ float4 LoadPx(const float* px, size_t i) {
  if (NCH == 4) return ((const float4*)px)[i];
  if (NCH == 3) { const float* p = px + i * 3; return make_float4(p[0], p[1], p[2], 0.f); }
  if (NCH == 2) { const float2 p = ((const float2*)px)[i]; return make_float4(p.x, p.y, 0.f, 0.f); }
  return make_float4(px[i], 0.f, 0.f, 0.f);
}
template <int NCH>
__device__ __forceinline__ void StorePx(float* px, size_t i, float4 v) {
  if (NCH == 4) ((float4*)px)[i] = v;
  else if (NCH == 3) { float* p = px + i * 3; p[0] = v.x; p[1] = v.y; p[2] = v.z; }
  else if (NCH == 2) ((float2*)px)[i] = make_float2(v.x, v.y);
  else px[i] = v.x;
}

// One channel under patch blend mode `mode`: `nw` / `an` the atlas sample and alpha, `old` / `ao` the frame's.  The Above modes are
// compose_kernel's BlendSample with (new = atlas, old = frame), the Below modes the same with the two swapped.
__device__ __forceinline__ float PatchSample(int mode, bool is_alpha, bool premul, bool clamp, float nw, float an, float old, float ao) {
  if (mode == 0) return old;
  if (mode == 1) return nw;
  if (mode == 2) return old + nw;
  if (mode == 3) return old * (clamp ? Clamp01(nw) : nw);
  const bool below = (mode & 1) != 0;   // 5 BlendBelow, 7 AlphaWeightedAddBelow
  const float n = below ? old : nw, o = below ? nw : old;
  float a = below ? ao : an;
  const float ob = below ? an : ao;
  if (clamp) a = Clamp01(a);
  if (mode <= 5) {   // kBlend
    if (is_alpha) return a + ob * (1.f - a);
    if (premul) return n + o * (1.f - a);
    const float A = a + ob * (1.f - a);
    return A == 0.f ? 0.f : (n * a + o * ob * (1.f - a)) / A;
  }
  return is_alpha ? o : o + n * a;   // kAlphaWeightedAdd
}

// a condition that is the same in every lane of the wavefront (it depends on the wavefront's row only), as a scalar branch
__device__ __forceinline__ bool Uniform(bool c) { return __builtin_amdgcn_readfirstlane((int)c) != 0; }

template <int NCH>
__device__ __forceinline__ void PatchTileBody(const PatchTile& t, const PatchFrame& fr, const int32_t* __restrict__ list,
                                              const PatchPos* __restrict__ pos, const PatchRef* __restrict__ refs) {
  constexpr int kRows = kPatchTile / 4;
  const int ai = fr.has_alpha ? NCH - 1 : -1;
  const bool premul = fr.premul != 0;
  const int x = (t.x0 & ~(kPatchTile - 1)) + ((int)threadIdx.x & 63);
  if (x < t.x0 || x >= t.x1) return;   // outside the box (no workgroup barrier follows)
  const int y0 = (t.y0 & ~(kPatchTile - 1)) + ((int)threadIdx.x >> 6);   // this wavefront's rows: y0 + 4 r
  float4 v[kRows];
#pragma unroll
  for (int r = 0; r < kRows; r++)
    if (Uniform(y0 + 4 * r >= t.y0 && y0 + 4 * r < t.y1)) v[r] = LoadPx<NCH>(fr.px, (size_t)(y0 + 4 * r) * fr.w + x);
  uint32_t touched = 0;
  for (int k = 0; k < t.count; k++) {
    const PatchPos p = pos[list[t.first + k]];
    const PatchRef rf = refs[p.ref];
    const int dx = x - p.x;
    const bool in_x = dx >= 0 && dx < rf.w;
    // the position's rows first (independent loads in flight), then the blends
    float4 a[kRows];
#pragma unroll
    for (int r = 0; r < kRows; r++) {
      const int dy = y0 + 4 * r - p.y;
      if (Uniform(dy >= 0 && dy < rf.h) && in_x) a[r] = LoadPx<NCH>(rf.px, (size_t)dy * rf.stride + dx);
    }
#pragma unroll
    for (int r = 0; r < kRows; r++) {
      const int dy = y0 + 4 * r - p.y;
      if (!Uniform(dy >= 0 && dy < rf.h) || !in_x) continue;
      const float4 o = v[r], n = a[r];
      const float ao = ai >= 0 ? Lane(o, ai) : 1.f, an = ai >= 0 ? Lane(n, ai) : 1.f;
      float res[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < NCH; c++) {
        const int g = c == ai ? 1 : 0;
        res[c] = PatchSample(p.mode[g], c == ai, premul, p.clamp[g] != 0, Lane(n, c), an, Lane(o, c), ao);
      }
      v[r] = make_float4(res[0], res[1], res[2], res[3]);
      touched |= 1u << r;
    }
  }
#pragma unroll
  for (int r = 0; r < kRows; r++)
    if (touched & (1u << r)) StorePx<NCH>(fr.px, (size_t)(y0 + 4 * r) * fr.w + x, v[r]);
}

__global__ __launch_bounds__(256) void patch_kernel(const PatchFrame* __restrict__ frames, const PatchTile* __restrict__ tiles,
                                                    const int32_t* __restrict__ list, const PatchPos* __restrict__ pos,
                                                    const PatchRef* __restrict__ refs) {
  const PatchTile& t = tiles[blockIdx.x];
  const PatchFrame& fr = frames[t.frame];
  switch (fr.nch) {   // uniform per workgroup: each variant is straight-line code for its channel count
    case 4: PatchTileBody<4>(t, fr, list, pos, refs); break;
    case 3: PatchTileBody<3>(t, fr, list, pos, refs); break;
    case 2: PatchTileBody<2>(t, fr, list, pos, refs); break;
    default: PatchTileBody<1>(t, fr, list, pos, refs); break;
  }
}

}  // namespace

void LaunchPatches(const PatchFrame* frames, const PatchTile* tiles, int ntiles, const int32_t* list, const PatchPos* pos, const PatchRef* refs,
                   hipStream_t s) {
  if (ntiles <= 0) return;
  hipLaunchKernelGGL(patch_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, frames, tiles, list, pos, refs);
}

}  // namespace jxlhip
