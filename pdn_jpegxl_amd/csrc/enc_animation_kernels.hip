// HIP kernels (gfx950) of animation encode: what changed between consecutive frames - as one box per pair
// (anim_extents_kernel, max_rects = 1) or as a box per pair and 64 x 64 tile (anim_tiles_kernel, further down, max_rects >= 2).  With a
// tolerance for "unchanged", at the end: one frame against the reference canvas per tile (anim_tiles_tol_kernel), and the canvas taking
// the rectangles that were written (anim_apply_rects_kernel).
//
// anim_extents_kernel: for every pair (frame k - 1, frame k) the bounding box of the samples whose BITS differ (+0.0 and -0.0 differ,
// equal NaN patterns do not, a changed alpha sample counts like any other).  It reads the caller's memory as it lies: any base
// pointer a sample allows, any row stride, rows of row_bytes bytes - the bytes between the end of a row and the next row are never
// loaded.  A sample differs when one of its bytes does, so the rows are compared as bytes and the first and the last differing byte
// of a row give the box; only the final division by the pixel size knows about pixels.
//
// One launch, grid = pairs x row blocks (a 2-frame 4K animation is 540 workgroups).  A wavefront takes a row at a time: the bytes in
// front of the first 16-byte boundary of frame k - 1's row (the head) and behind the last (the tail) go one byte per lane; the middle
// goes 16 bytes per lane and step: frame k - 1 in aligned 16-byte loads, frame k in 16-byte loads at the same offset, aligned when
// the two rows are congruent modulo 16 and unaligned otherwise (global loads of gfx950 take any address).  Lanes
// keep (first byte, last byte, first row, last row) in registers; a wavefront reduces them by shuffles, the workgroup through 64
// bytes of LDS, and one lane issues at most four atomics (unsigned min for x0 / y0, signed max for x1 / y1) - none when the
// workgroup saw no difference.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include "enc_animation.h"

namespace jxlhip {
namespace {

constexpr int kExtThreads = 256, kExtWaves = kExtThreads / 64;

struct ExtAcc {
  uint64_t lo = ~(uint64_t)0, hi = 0;   // first and last differing byte of a row, over the rows seen
  int32_t y0 = 0x7FFFFFFF, y1 = -1;     // y1 < 0: no difference seen
  __device__ __forceinline__ void Mark(uint64_t first, uint64_t last, int32_t y) {
    lo = first < lo ? first : lo;
    hi = last > hi ? last : hi;
    y0 = y < y0 ? y : y0;
    y1 = y > y1 ? y : y1;
  }
};

__device__ __forceinline__ uint32_t FirstByte(uint32_t d) { return (uint32_t)(__ffs((int)d) - 1) >> 3; }   // d != 0
__device__ __forceinline__ uint32_t LastByte(uint32_t d) { return (31u - (uint32_t)__clz((int)d)) >> 3; }

__device__ __forceinline__ void MarkChunk(const uint4& a, const uint4& b, uint64_t off, int32_t y, ExtAcc& acc) {
  const uint32_t d0 = a.x ^ b.x, d1 = a.y ^ b.y, d2 = a.z ^ b.z, d3 = a.w ^ b.w;
  if ((d0 | d1 | d2 | d3) == 0) return;
  const uint32_t first = d0 ? FirstByte(d0) : (d1 ? 4 + FirstByte(d1) : (d2 ? 8 + FirstByte(d2) : 12 + FirstByte(d3)));
  const uint32_t last = d3 ? 12 + LastByte(d3) : (d2 ? 8 + LastByte(d2) : (d1 ? 4 + LastByte(d1) : LastByte(d0)));
  acc.Mark(off + first, off + last, y);
}

// 16 bytes at p, whatever its alignment (global loads of gfx950 need none: this is one dwordx4 load)
__device__ __forceinline__ uint4 LoadUnaligned(const uint8_t* p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

// the middle of a row: chunks [0, nmid) of 16 bytes at a (16-byte aligned) against those at b; `off`: of a within its row
__device__ __forceinline__ void CompareMiddle(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint64_t nmid, uint64_t off, int lane,
                                              int32_t y, ExtAcc& acc) {
#pragma unroll 4
  for (uint64_t j = (uint64_t)lane; j < nmid; j += 64) {
    const uint4 va = *reinterpret_cast<const uint4*>(a + 16 * j);
    const uint4 vb = LoadUnaligned(b + 16 * j);
    MarkChunk(va, vb, off + 16 * j, y, acc);
  }
}

__global__ __launch_bounds__(kExtThreads) void anim_extents_kernel(const AnimFrameSrc* __restrict__ frames, int32_t h, uint64_t row_bytes,
                                                                    uint32_t pixel_bytes, int32_t rows_per_wg, uint32_t row_blocks,
                                                                    AnimExtent* __restrict__ out) {
  const uint32_t pair = blockIdx.x / row_blocks, block = blockIdx.x % row_blocks;
  const AnimFrameSrc fa = frames[pair], fb = frames[pair + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row0 = (int64_t)block * rows_per_wg;
  const int32_t row1 = (int32_t)std::min<int64_t>(h, row0 + rows_per_wg);
  ExtAcc acc;
  for (int32_t y = (int32_t)row0 + wave; y < row1; y += kExtWaves) {
    const uint8_t* a = fa.data + (int64_t)y * fa.stride;
    const uint8_t* b = fb.data + (int64_t)y * fb.stride;
    // [0, head) and [tail, row_bytes): a byte per lane; [head, tail): 16 bytes per lane and step.  Every load lies inside the row.
    const uint64_t head = std::min<uint64_t>(row_bytes, (uint64_t)(-(intptr_t)a & 15));
    const uint64_t nmid = (row_bytes - head) >> 4;
    const uint64_t tail = head + 16 * nmid;
    if ((uint64_t)lane < head) {
      if (a[lane] != b[lane]) acc.Mark((uint64_t)lane, (uint64_t)lane, y);
    } else if (lane >= 32 && lane < 48 && tail + (uint64_t)(lane - 32) < row_bytes) {
      const uint64_t o = tail + (uint64_t)(lane - 32);
      if (a[o] != b[o]) acc.Mark(o, o, y);
    }
    CompareMiddle(a + head, b + head, nmid, head, lane, y, acc);
  }
  // bytes -> pixels, then lanes -> wavefront -> workgroup -> at most four atomics
  uint32_t x0 = 0xFFFFFFFFu, y0 = 0xFFFFFFFFu;
  int32_t x1 = -1, y1 = -1;
  if (acc.y1 >= 0) {
    x0 = (uint32_t)(acc.lo / pixel_bytes);
    x1 = (int32_t)(acc.hi / pixel_bytes);
    y0 = (uint32_t)acc.y0;
    y1 = acc.y1;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    x0 = std::min(x0, (uint32_t)__shfl_xor((int)x0, m, 64));
    y0 = std::min(y0, (uint32_t)__shfl_xor((int)y0, m, 64));
    x1 = std::max(x1, __shfl_xor(x1, m, 64));
    y1 = std::max(y1, __shfl_xor(y1, m, 64));
  }
  __shared__ int32_t part[kExtWaves][4];
  if (lane == 0) { part[wave][0] = (int32_t)x0; part[wave][1] = (int32_t)y0; part[wave][2] = x1; part[wave][3] = y1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kExtWaves; w++) {
      x0 = std::min(x0, (uint32_t)part[w][0]);
      y0 = std::min(y0, (uint32_t)part[w][1]);
      x1 = std::max(x1, part[w][2]);
      y1 = std::max(y1, part[w][3]);
    }
    if (y1 >= 0) {
      AnimExtent* e = out + pair;
      atomicMin(reinterpret_cast<unsigned int*>(&e->x0), x0);
      atomicMin(reinterpret_cast<unsigned int*>(&e->y0), y0);
      atomicMax(&e->x1, x1);
      atomicMax(&e->y1, y1);
    }
  }
}

// ---- anim_tiles_kernel: the same measurement per 64 x 64-pixel tile of the canvas, for max_rects >= 2 (enc_animation.h: AnimFrameRects).
//
// One launch, grid = pairs x tile rows x column groups.  A workgroup owns one tile row (up to 64 canvas rows) of a group of whole tile
// columns; a lane owns the 16-byte chunk [16 c, 16 c + 16) of a row, counted from the ROW'S START, and walks down the rows, eight rows
// of both frames loaded before any is looked at.  A tile is 64 pixel_bytes bytes wide - a multiple of 16 for every pixel size - so tile
// boundaries are chunk boundaries and a chunk lies in exactly one tile: the lane keeps one (first byte, last byte, first row, last row)
// in registers, relative to its tile.  A row step of a wavefront is one contiguous 1 KB read per frame, aligned when the caller's rows
// are.  The chunk that the end of the row cuts is loaded as the LAST 16 bytes of the row and the bytes in front of the chunk are masked
// off (rows shorter than 16 bytes: a byte at a time, by one thread): no byte outside a row is loaded.  At the end the lanes that saw a
// difference fold into an LDS table of the band's tiles (four LDS atomics each), and one thread per tile stores the packed word:
// every word of the table is written, by exactly one workgroup, with a plain store - no global atomics, no memset beforehand.
constexpr int kTileThreads = 256, kTileRowsInFlight = 8;

struct TileAcc {
  uint32_t lo = 0xFFFFFFFFu, hi = 0, y0 = 0xFFFFFFFFu, y1 = 0;   // bytes relative to the tile's first, rows to its first; lo > hi: nothing seen
  __device__ __forceinline__ void Mark(uint32_t first, uint32_t last, uint32_t y) {
    lo = first < lo ? first : lo;
    hi = last > hi ? last : hi;
    y0 = y < y0 ? y : y0;
    y1 = y > y1 ? y : y1;
  }
};

// The 16 bytes a and b were loaded from byte `base` of their tile (base + skip: the chunk's first byte; the `skip` bytes in front of it
// belong to the chunk before and are ignored).
__device__ __forceinline__ void MarkTileChunk(const uint4& a, const uint4& b, uint32_t base, uint32_t skip, uint32_t y, TileAcc& acc) {
  uint32_t d[4] = {a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w};
  if ((d[0] | d[1] | d[2] | d[3]) == 0) return;
  if (skip) {
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
      if (4 * i + 4 <= skip) d[i] = 0;
      else if (4 * i < skip) d[i] &= ~0u << (8 * (skip - 4 * i));
    }
    if ((d[0] | d[1] | d[2] | d[3]) == 0) return;
  }
  const uint32_t first = d[0] ? FirstByte(d[0]) : (d[1] ? 4 + FirstByte(d[1]) : (d[2] ? 8 + FirstByte(d[2]) : 12 + FirstByte(d[3])));
  const uint32_t last = d[3] ? 12 + LastByte(d[3]) : (d[2] ? 8 + LastByte(d[2]) : (d[1] ? 4 + LastByte(d[1]) : LastByte(d[0])));
  acc.Mark(base + first, base + last, y);
}

__global__ __launch_bounds__(kTileThreads) void anim_tiles_kernel(const AnimFrameSrc* __restrict__ frames, int32_t h, uint64_t row_bytes, uint32_t pixel_bytes,
                                                                  uint32_t tiles_x, uint32_t tiles_y, uint32_t group_tiles, uint32_t groups,
                                                                  uint32_t* __restrict__ out) {
  const uint32_t group = blockIdx.x % groups, ty = (blockIdx.x / groups) % tiles_y, pair = blockIdx.x / groups / tiles_y;
  const AnimFrameSrc fa = frames[pair], fb = frames[pair + 1];
  const uint32_t tid = threadIdx.x;
  const uint32_t tile_chunks = 4 * pixel_bytes;                  // 64 pixel_bytes / 16
  const uint32_t local = tid / tile_chunks;                      // the lane's tile within the group; >= group_tiles: the lane idles
  const uint64_t chunk = (uint64_t)group * group_tiles * tile_chunks + tid;
  const uint32_t rows = (uint32_t)std::min<int64_t>(kAnimTile, (int64_t)h - (int64_t)ty * kAnimTile);
  __shared__ uint32_t table[kTileThreads / 4][4];                // per tile of the group: first byte, first row (min), last byte, last row (max)
  if (tid < kTileThreads / 4) { table[tid][0] = 0xFFFFFFFFu; table[tid][1] = 0xFFFFFFFFu; table[tid][2] = 0; table[tid][3] = 0; }
  __syncthreads();
  TileAcc acc;
  const int64_t row0 = (int64_t)ty * kAnimTile;
  if (row_bytes < 16) {
    // a row of fewer than 16 bytes (one tile column, at most 15 pixels wide): a byte at a time
    if (group == 0 && tid == 0) {
      for (uint32_t y = 0; y < rows; y++) {
        const uint8_t* a = fa.data + (row0 + y) * fa.stride;
        const uint8_t* b = fb.data + (row0 + y) * fb.stride;
        for (uint32_t i = 0; i < (uint32_t)row_bytes; i++)
          if (a[i] != b[i]) acc.Mark(i, i, y);
      }
    }
  } else if (local < group_tiles && 16 * chunk < row_bytes) {
    // where the lane loads: its chunk, or - the chunk the row's end cuts - the last 16 bytes of the row, `skip` bytes earlier
    const uint64_t at = std::min<uint64_t>(16 * chunk, row_bytes - 16);
    const uint32_t skip = (uint32_t)(16 * chunk - at);
    const uint32_t base = (tid % tile_chunks) * 16 - skip;       // of the load within the tile (mod 2^32 where skip reaches back; first >= skip mends it)
    const uint8_t* a = fa.data + row0 * fa.stride + at;
    const uint8_t* b = fb.data + row0 * fb.stride + at;
    uint32_t y = 0;
    for (; y + kTileRowsInFlight <= rows; y += kTileRowsInFlight) {
      uint4 va[kTileRowsInFlight], vb[kTileRowsInFlight];
#pragma unroll
      for (int r = 0; r < kTileRowsInFlight; r++) {
        va[r] = LoadUnaligned(a + (int64_t)r * fa.stride);
        vb[r] = LoadUnaligned(b + (int64_t)r * fb.stride);
      }
#pragma unroll
      for (int r = 0; r < kTileRowsInFlight; r++) MarkTileChunk(va[r], vb[r], base, skip, y + r, acc);
      a += (int64_t)kTileRowsInFlight * fa.stride;
      b += (int64_t)kTileRowsInFlight * fb.stride;
    }
    for (; y < rows; y++) {
      MarkTileChunk(LoadUnaligned(a), LoadUnaligned(b), base, skip, y, acc);
      a += fa.stride;
      b += fb.stride;
    }
  }
  if (acc.lo <= acc.hi) {
    const uint32_t t = row_bytes < 16 ? 0 : local;
    atomicMin(&table[t][0], acc.lo);
    atomicMin(&table[t][1], acc.y0);
    atomicMax(&table[t][2], acc.hi);
    atomicMax(&table[t][3], acc.y1);
  }
  __syncthreads();
  const uint64_t tx = (uint64_t)group * group_tiles + tid;
  if (tid < group_tiles && tx < tiles_x) {
    uint32_t word = kAnimTileEmpty;
    if (table[tid][0] != 0xFFFFFFFFu) word = table[tid][0] / pixel_bytes | table[tid][1] << 8 | (table[tid][2] / pixel_bytes) << 16 | table[tid][3] << 24;
    out[((uint64_t)pair * tiles_y + ty) * tiles_x + tx] = word;
  }
}

// ---- anim_tiles_tol_kernel: the tile table of ONE frame against the reference canvas R under a tolerance (enc_animation.h:
// AnimSampleChanged; DESIGN.md §2 "Animation encode").  The skeleton is anim_tiles_kernel's - a workgroup per tile row and group of whole
// tile columns, a lane per 16-byte chunk counted from the row's start (sample-aligned for 1-, 2- and 4-byte samples whatever the pixel
// size), eight rows of both operands loaded before any is looked at, the chunk the row's end cuts loaded as the row's last 16 bytes, rows
// under 16 bytes by one thread, one LDS table, one plain store per tile word - and only "differs" is another thing: instead of a XOR b,
// a comparator per sample type gives the four dwords in which every byte of a changed sample is 0xFF, and MarkTileChunk takes them from
// there.  The frame's rows have any stride and any sample-aligned base; R's rows are tight.  No byte outside a row is loaded.
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));

// Per 16-bit half of a dword: 0xFFFF where |a - b| > tol (tol2: tol in both halves), packed arithmetic throughout
__device__ __forceinline__ uint32_t Over16(uint32_t a, uint32_t b, uint32_t tol2) {
  u16x2 va, vb, vt;
  __builtin_memcpy(&va, &a, 4);
  __builtin_memcpy(&vb, &b, 4);
  __builtin_memcpy(&vt, &tol2, 4);
  const u16x2 d = __builtin_elementwise_max(va, vb) - __builtin_elementwise_min(va, vb);
  const u16x2 over = __builtin_elementwise_sub_sat(d, vt);           // > 0 where the half moved by more than tol
  const u16x2 m = (u16x2){0, 0} - __builtin_elementwise_min(over, (u16x2){1, 1});
  uint32_t out;
  __builtin_memcpy(&out, &m, 4);
  return out;
}

// Per byte of a dword: 0xFF where |a - b| > tol - the even and the odd bytes as two dwords of 16-bit halves
__device__ __forceinline__ uint32_t Over8(uint32_t a, uint32_t b, uint32_t tol2) {
  const uint32_t even = Over16(a & 0x00FF00FFu, b & 0x00FF00FFu, tol2) & 0x00FF00FFu;
  const uint32_t odd = Over16(a >> 8 & 0x00FF00FFu, b >> 8 & 0x00FF00FFu, tol2) & 0x00FF00FFu;
  return even | odd << 8;
}

// The dword of "changed" bytes of one dword of samples.  tol: floor(tolerance) in both halves (integers), the tolerance's bits (floats).
template <int KIND> __device__ __forceinline__ uint32_t ChangedDword(uint32_t a, uint32_t b, uint32_t tol) {
  if (KIND == kAnimU8) return Over8(a, b, tol);
  if (KIND == kAnimU16) return Over16(a, b, tol);
  if (a == b) return 0;
  const float t = __uint_as_float(tol);
  if (KIND == kAnimF32) return AnimFloatChanged(a, b, t) ? 0xFFFFFFFFu : 0u;
  return (AnimHalfChanged(a & 0xFFFFu, b & 0xFFFFu, t) ? 0x0000FFFFu : 0u) | (AnimHalfChanged(a >> 16, b >> 16, t) ? 0xFFFF0000u : 0u);
}

template <int KIND>
__device__ __forceinline__ void MarkTileChunkTol(const uint4& a, const uint4& b, uint32_t tol, uint32_t base, uint32_t skip, uint32_t y, TileAcc& acc) {
  if (((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) == 0) return;   // equal bits are unchanged for every sample type
  const uint4 d = {ChangedDword<KIND>(a.x, b.x, tol), ChangedDword<KIND>(a.y, b.y, tol), ChangedDword<KIND>(a.z, b.z, tol), ChangedDword<KIND>(a.w, b.w, tol)};
  MarkTileChunk(d, uint4{0, 0, 0, 0}, base, skip, y, acc);                       // (d ^ 0: the first and last marked byte, `skip` honoured)
}

template <int KIND>
__global__ __launch_bounds__(kTileThreads) void anim_tiles_tol_kernel(AnimFrameSrc fa, const uint8_t* __restrict__ ref, int32_t h, uint64_t row_bytes,
                                                                      uint32_t pixel_bytes, uint32_t tiles_x, uint32_t tiles_y, uint32_t group_tiles,
                                                                      uint32_t groups, float tolerance, uint32_t* __restrict__ out) {
  constexpr uint32_t kSampleBytes = KIND == kAnimU8 ? 1 : (KIND == kAnimF32 ? 4 : 2);
  const uint32_t group = blockIdx.x % groups, ty = blockIdx.x / groups;
  const AnimFrameSrc fb{ref, (int64_t)row_bytes};
  const uint32_t int_tol = AnimIntTolerance(tolerance);
  const uint32_t tol = KIND == kAnimU8 || KIND == kAnimU16 ? int_tol | int_tol << 16 : __float_as_uint(tolerance);
  const uint32_t tid = threadIdx.x;
  const uint32_t tile_chunks = 4 * pixel_bytes;                  // 64 pixel_bytes / 16
  const uint32_t local = tid / tile_chunks;                      // the lane's tile within the group; >= group_tiles: the lane idles
  const uint64_t chunk = (uint64_t)group * group_tiles * tile_chunks + tid;
  const uint32_t rows = (uint32_t)std::min<int64_t>(kAnimTile, (int64_t)h - (int64_t)ty * kAnimTile);
  __shared__ uint32_t table[kTileThreads / 4][4];                // per tile of the group: first byte, first row (min), last byte, last row (max)
  if (tid < kTileThreads / 4) { table[tid][0] = 0xFFFFFFFFu; table[tid][1] = 0xFFFFFFFFu; table[tid][2] = 0; table[tid][3] = 0; }
  __syncthreads();
  TileAcc acc;
  const int64_t row0 = (int64_t)ty * kAnimTile;
  if (row_bytes < 16) {
    // a row of fewer than 16 bytes (one tile column): a sample at a time, by the rule itself
    if (group == 0 && tid == 0) {
      for (uint32_t y = 0; y < rows; y++) {
        const uint8_t* a = fa.data + (row0 + y) * fa.stride;
        const uint8_t* b = fb.data + (row0 + y) * fb.stride;
        for (uint32_t i = 0; i < (uint32_t)row_bytes; i += kSampleBytes) {
          uint32_t sa = 0, sb = 0;
          __builtin_memcpy(&sa, a + i, kSampleBytes);
          __builtin_memcpy(&sb, b + i, kSampleBytes);
          if (AnimSampleChanged((AnimSample)KIND, sa, sb, tolerance)) acc.Mark(i, i + kSampleBytes - 1, y);
        }
      }
    }
  } else if (local < group_tiles && 16 * chunk < row_bytes) {
    // where the lane loads: its chunk, or - the chunk the row's end cuts - the last 16 bytes of the row, `skip` bytes earlier (row_bytes
    // and 16 are multiples of the sample size: so is skip)
    const uint64_t at = std::min<uint64_t>(16 * chunk, row_bytes - 16);
    const uint32_t skip = (uint32_t)(16 * chunk - at);
    const uint32_t base = (tid % tile_chunks) * 16 - skip;       // of the load within the tile (mod 2^32 where skip reaches back; first >= skip mends it)
    const uint8_t* a = fa.data + row0 * fa.stride + at;
    const uint8_t* b = fb.data + row0 * fb.stride + at;
    uint32_t y = 0;
    for (; y + kTileRowsInFlight <= rows; y += kTileRowsInFlight) {
      uint4 va[kTileRowsInFlight], vb[kTileRowsInFlight];
#pragma unroll
      for (int r = 0; r < kTileRowsInFlight; r++) {
        va[r] = LoadUnaligned(a + (int64_t)r * fa.stride);
        vb[r] = LoadUnaligned(b + (int64_t)r * fb.stride);
      }
#pragma unroll
      for (int r = 0; r < kTileRowsInFlight; r++) MarkTileChunkTol<KIND>(va[r], vb[r], tol, base, skip, y + r, acc);
      a += (int64_t)kTileRowsInFlight * fa.stride;
      b += (int64_t)kTileRowsInFlight * fb.stride;
    }
    for (; y < rows; y++) {
      MarkTileChunkTol<KIND>(LoadUnaligned(a), LoadUnaligned(b), tol, base, skip, y, acc);
      a += fa.stride;
      b += fb.stride;
    }
  }
  if (acc.lo <= acc.hi) {
    const uint32_t t = row_bytes < 16 ? 0 : local;
    atomicMin(&table[t][0], acc.lo);
    atomicMin(&table[t][1], acc.y0);
    atomicMax(&table[t][2], acc.hi);
    atomicMax(&table[t][3], acc.y1);
  }
  __syncthreads();
  const uint64_t tx = (uint64_t)group * group_tiles + tid;
  if (tid < group_tiles && tx < tiles_x) {
    uint32_t word = kAnimTileEmpty;
    if (table[tid][0] != 0xFFFFFFFFu) word = table[tid][0] / pixel_bytes | table[tid][1] << 8 | (table[tid][2] / pixel_bytes) << 16 | table[tid][3] << 24;
    out[(uint64_t)ty * tiles_x + tx] = word;
  }
}

// ---- anim_apply_rects_kernel: R takes the frame's pixels inside the rectangles that were written - what a decoder replaces.  grid =
// (row blocks of the highest rectangle, rectangles); a wavefront copies a row of a rectangle at a time: the bytes in front of R's first
// 16-byte boundary and behind its last go one byte per lane, the middle 16 bytes per lane and step - R stored aligned, the frame loaded
// at the same offset whatever its alignment.  The rectangles are disjoint and lie inside the canvas: no byte outside them is touched.
constexpr int kApplyThreads = 256, kApplyWaves = kApplyThreads / 64;

struct AnimRectList { AnimRect r[kAnimMaxRects]; };

__global__ __launch_bounds__(kApplyThreads) void anim_apply_rects_kernel(AnimFrameSrc frame, uint8_t* __restrict__ ref, uint64_t row_bytes, uint32_t pixel_bytes,
                                                                         AnimRectList rects) {
  const AnimRect r = rects.r[blockIdx.y];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t y = (int64_t)blockIdx.x * kApplyWaves + wave;      // of the rectangle
  if (y >= r.h) return;
  const uint64_t n = (uint64_t)r.w * pixel_bytes, x_off = (uint64_t)r.x * pixel_bytes;
  const uint8_t* s = frame.data + (r.y + y) * frame.stride + x_off;
  uint8_t* d = ref + (uint64_t)(r.y + y) * row_bytes + x_off;
  const uint64_t head = std::min<uint64_t>(n, (uint64_t)(-(intptr_t)d & 15));
  const uint64_t nmid = (n - head) >> 4;
  const uint64_t tail = head + 16 * nmid;
  if ((uint64_t)lane < head) {
    d[lane] = s[lane];
  } else if (lane >= 32 && lane < 48 && tail + (uint64_t)(lane - 32) < n) {
    const uint64_t o = tail + (uint64_t)(lane - 32);
    d[o] = s[o];
  }
#pragma unroll 4
  for (uint64_t j = (uint64_t)lane; j < nmid; j += 64) *reinterpret_cast<uint4*>(d + head + 16 * j) = LoadUnaligned(s + head + 16 * j);
}

}  // namespace

void LaunchAnimTilesTol(AnimFrameSrc frame, const uint8_t* ref, int32_t w, int32_t h, uint32_t pixel_bytes, AnimSample kind, float tolerance,
                        uint32_t* out, void* stream) {
  if (w <= 0 || h <= 0 || pixel_bytes < 1 || pixel_bytes > 16) return;
  const uint32_t tiles_x = AnimTilesAcross(w), tiles_y = AnimTilesAcross(h);
  const uint32_t group_tiles = (kTileThreads / 4) / pixel_bytes;           // as LaunchAnimTiles
  const uint32_t groups = (tiles_x + group_tiles - 1) / group_tiles;
  const dim3 grid(tiles_y * groups), block(kTileThreads);                  // (at most 2^24 x 2^20 / 4 tiles of 2^30 pixels: far below 2^31)
  const uint64_t row_bytes = (uint64_t)w * pixel_bytes;
  hipStream_t s = (hipStream_t)stream;
  switch (kind) {
    case kAnimU8: hipLaunchKernelGGL(anim_tiles_tol_kernel<kAnimU8>, grid, block, 0, s, frame, ref, h, row_bytes, pixel_bytes, tiles_x, tiles_y, group_tiles, groups, tolerance, out); break;
    case kAnimU16: hipLaunchKernelGGL(anim_tiles_tol_kernel<kAnimU16>, grid, block, 0, s, frame, ref, h, row_bytes, pixel_bytes, tiles_x, tiles_y, group_tiles, groups, tolerance, out); break;
    case kAnimF16: hipLaunchKernelGGL(anim_tiles_tol_kernel<kAnimF16>, grid, block, 0, s, frame, ref, h, row_bytes, pixel_bytes, tiles_x, tiles_y, group_tiles, groups, tolerance, out); break;
    case kAnimF32: hipLaunchKernelGGL(anim_tiles_tol_kernel<kAnimF32>, grid, block, 0, s, frame, ref, h, row_bytes, pixel_bytes, tiles_x, tiles_y, group_tiles, groups, tolerance, out); break;
  }
}

void LaunchAnimApplyRects(AnimFrameSrc frame, uint8_t* ref, int32_t w, uint32_t pixel_bytes, const AnimRect* rects, int32_t nrects, void* stream) {
  if (nrects < 1 || nrects > kAnimMaxRects || w <= 0) return;
  AnimRectList list;
  int32_t highest = 0;
  for (int32_t i = 0; i < kAnimMaxRects; i++) {
    list.r[i] = i < nrects ? rects[i] : AnimRect{0, 0, 0, 0};
    highest = std::max(highest, list.r[i].h);
  }
  if (highest <= 0) return;
  hipLaunchKernelGGL(anim_apply_rects_kernel, dim3((uint32_t)((highest + kApplyWaves - 1) / kApplyWaves), (uint32_t)nrects), dim3(kApplyThreads), 0,
                     (hipStream_t)stream, frame, ref, (uint64_t)w * pixel_bytes, pixel_bytes, list);
}

void LaunchAnimTiles(const AnimFrameSrc* frames, int32_t npairs, int32_t w, int32_t h, uint32_t pixel_bytes, uint32_t* out, void* stream) {
  if (npairs <= 0 || w <= 0 || h <= 0 || pixel_bytes < 1 || pixel_bytes > 16) return;
  const uint32_t tiles_x = AnimTilesAcross(w), tiles_y = AnimTilesAcross(h);
  const uint32_t group_tiles = (kTileThreads / 4) / pixel_bytes;           // whole tiles of 4 pixel_bytes chunks that 256 lanes hold: 64 .. 4
  const uint32_t groups = (tiles_x + group_tiles - 1) / group_tiles;
  // one launch, unless the grid would pass 2^30 workgroups: then some pairs at a time
  const int64_t per_pair = (int64_t)tiles_y * groups;
  const int32_t pairs_per_launch = (int32_t)std::max<int64_t>(1, std::min<int64_t>(npairs, ((int64_t)1 << 30) / per_pair));
  for (int32_t p = 0; p < npairs; p += pairs_per_launch) {
    const int32_t cnt = std::min(pairs_per_launch, npairs - p);
    hipLaunchKernelGGL(anim_tiles_kernel, dim3((uint32_t)(cnt * per_pair)), dim3(kTileThreads), 0, (hipStream_t)stream, frames + p, h,
                       (uint64_t)w * pixel_bytes, pixel_bytes, tiles_x, tiles_y, group_tiles, groups, out + (size_t)p * tiles_x * tiles_y);
  }
}

void LaunchAnimExtents(const AnimFrameSrc* frames, int32_t npairs, int32_t h, uint64_t row_bytes, uint32_t pixel_bytes, AnimExtent* out, void* stream) {
  if (npairs <= 0 || h <= 0) return;
  // a row per wavefront at least; more rows per workgroup once the grid has some thousand workgroups, and whatever keeps it below 2^30
  const int64_t rows = (int64_t)npairs * h;
  int64_t per_wg = std::max<int64_t>(kExtWaves, std::min<int64_t>(64, rows / 4096));
  per_wg = std::max(per_wg, (rows + (1 << 30) - 1) >> 30);
  per_wg = std::min<int64_t>((per_wg + kExtWaves - 1) / kExtWaves * kExtWaves, 0x7FFFFFFF / 2);
  const uint32_t row_blocks = (uint32_t)((h + per_wg - 1) / per_wg);
  hipLaunchKernelGGL(anim_extents_kernel, dim3((uint32_t)npairs * row_blocks), dim3(kExtThreads), 0, (hipStream_t)stream, frames, h, row_bytes, pixel_bytes,
                     (int32_t)per_wg, row_blocks, out);
}

}  // namespace jxlhip
