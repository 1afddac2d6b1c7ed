// Dynamic LDS of the four serial entropy kernels (entropy_kernels.hip) and of recon_tile_kernel (tile_kernels.hip), written once for
// both sides: the kernels carve their `extern __shared__` block through these descriptions, and the host (entropy_plan.cc, the
// Launch* wrappers) asks the same descriptions how many bytes a launch needs.  A layout is a plain struct of byte offsets computed
// from the numbers that determine it; `end` / `tables` is the first byte behind it.  Nothing here touches memory.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "dev_types.h"
#include "modular_rules.h"

namespace jxlhip {

#define JXL_LAYOUT __host__ __device__ __forceinline__

constexpr int kRingWords = 32;       // words of a lane's bit window in the LF, alpha and Modular decoders (LaneBits)
constexpr int kHfRingWords = 32;     // ... and in the HF decoder (one size: a 16-word variant paid off only while the coefficient orders lived in LDS)
constexpr int kModWindowLanes = 64;  // modular_ans_kernel lays its bit windows out for a whole wavefront whatever `lanes` is
constexpr int kNzColBytes = 96;      // HF decoder, per lane: non-zero counts of 32 columns x 3 channels
constexpr int kNnzCtxBytes = 64;     // HF decoder: the LDS copy of d_nnz_ctx
constexpr int kWpStateInts = WpState::kInts;     // weighted-predictor state: ints per column (of rb_width + 2 columns)
constexpr int kUniRows = 3;          // modular_uniform.h: rows the one-section-per-wavefront decoder keeps
constexpr size_t kUniGridBytes = (size_t)kUniGridCells * 16;   // ... and its grid of 16-byte leaf records
// The most dynamic LDS a launch asks for; tables that need more stay in global memory (the kLds = false variants).
constexpr size_t kLdsMax = 150 * 1024;

// Allowances the host adds to a size for the round-ups inside a layout (a layout's start is not known to be aligned when the size
// is asked for).  Their values decide on which side of the 80 KB / 160 KB budgets a frame falls: they do not change.
constexpr size_t kCodeAllowance = 8;     // the round-up to 8 in front of the alias tables (CodeLds).  It pays for that round-up in the HF
                                         // layout (the code follows the lanes' arrays); behind a tree (ModTablesLds: a 16-aligned
                                         // start, 16-byte nodes) the code is always aligned and the allowance pays for nothing
constexpr size_t kTreeAllowance = 16;    // the round-up to 16 in front of the tree (ModTablesLds); pays for nothing where the tree
                                         // follows bit windows (a multiple of 128 bytes)
constexpr size_t kHfTailAllowance = 32;  // behind the HF tables; pays for nothing (the layout ends with the 64 bytes of contexts)
constexpr int kHfEstimateLanes = 4;      // lanes the HF lane-stride heuristic counts beside a frame's tables

JXL_LAYOUT size_t LdsRoundUp(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }

// ---- a code's tables: alias | cfg | context map
struct CodeShape {
  uint32_t clusters, log_alpha, contexts;
  bool prefix;   // prefix codes have no alias tables
  JXL_LAYOUT uint32_t AliasEntries() const { return prefix ? 0u : clusters << log_alpha; }
};
JXL_LAYOUT CodeShape ShapeOf(const DevCode& dc) { return CodeShape{dc.num_clusters, dc.log_alpha, dc.num_ctx, (dc.slow & 1) != 0}; }
struct CodeLds {
  size_t alias, cfg, cmap, end;
  JXL_LAYOUT CodeLds(size_t off, const CodeShape& s) {
    alias = LdsRoundUp(off, 8);
    cfg = alias + (size_t)s.AliasEntries() * 8;
    cmap = cfg + (size_t)s.clusters * 4;
    end = cmap + s.contexts;
  }
};
JXL_LAYOUT size_t CodeLdsBytes(const CodeShape& s) { return kCodeAllowance + CodeLds(0, s).end; }

// ---- MA tree + Modular code (LoadModTables): tree | code
struct ModTablesLds {
  size_t tree, code, end;
  JXL_LAYOUT ModTablesLds(size_t off, size_t tree_nodes, const CodeShape& s) {
    tree = LdsRoundUp(off, 16);
    code = tree + tree_nodes * sizeof(DevTreeNode);
    end = CodeLds(code, s).end;
  }
};
JXL_LAYOUT size_t ModTablesLdsBytes(size_t tree_nodes, const CodeShape& s) { return kTreeAllowance + tree_nodes * sizeof(DevTreeNode) + CodeLdsBytes(s); }

// ---- lf_ans_kernel / alpha_ans_kernel: bit windows of `slots` lanes | tree + code
struct SlotsLds {
  size_t tables;   // = the whole of it for the variant that reads its tables from global memory
  JXL_LAYOUT explicit SlotsLds(int slots) { tables = (size_t)slots * kRingWords * 4; }
};
JXL_LAYOUT size_t SlotsLdsBytes(int slots, size_t tree_nodes, const CodeShape& s) { return SlotsLds(slots).tables + ModTablesLdsBytes(tree_nodes, s); }

// ---- alpha_ans_kernel, launches that finish groups in one pass (the lane path): the previous row of every lane's group as packed u8,
// behind the launch's tables (behind the bit windows when the tables stay in global memory).  Dword j of lane `slot` lies at
// rows[j * slots + slot], the bank-per-lane layout of the bit windows.
struct AlphaRowsLds {
  size_t rows, end;
  JXL_LAYOUT AlphaRowsLds(size_t tables_end, int slots) {
    rows = LdsRoundUp(tables_end, 4);
    end = rows + (size_t)slots * kGroupDim;
  }
};
// (no allowance for the round-up: the tables' allowances, kTreeAllowance and kCodeAllowance, pay for nothing behind bit windows)
JXL_LAYOUT size_t AlphaRowsLdsBytes(int slots) { return (size_t)slots * kGroupDim; }
static_assert(kTreeAllowance + kCodeAllowance >= 4, "the row area's round-up is paid for by the tables' allowances");

// ---- modular_ans_kernel: bit windows | previous-row buffers | weighted-predictor state | grid (uniform shape only) | tree + code
// uniform: the one-section-per-wavefront shape of modular_uniform.h (three rows and the leaf grid instead of one row per lane)
JXL_LAYOUT bool ModularUniform(int lanes, int rb_width) { return lanes == 1 && rb_width > 0; }
struct ModularLds {
  size_t rows, wp, wp_ints, grid, tables;
  JXL_LAYOUT ModularLds(int lanes, int rb_width, int wp_lds, bool uniform) {
    rows = (size_t)kModWindowLanes * kRingWords * 4;
    wp = rows + (size_t)(uniform ? kUniRows : lanes) * rb_width * 4;
    wp_ints = (size_t)kWpStateInts * (rb_width + 2);
    grid = wp + (wp_lds ? (size_t)lanes * wp_ints * 4 : 0);
    tables = grid + (uniform ? kUniGridBytes : 0);
  }
};
JXL_LAYOUT size_t ModularLdsBytes(int lanes, int rb_width, int wp_lds, bool uniform, size_t tree_nodes, const CodeShape& s) {
  return ModularLds(lanes, rb_width, wp_lds, uniform).tables + ModTablesLdsBytes(tree_nodes, s);
}

// ---- hf_decode_kernel: bit windows | descriptor queues | non-zero columns (each for `nslots` lanes) | code | non-zero contexts
constexpr int kHfQueueDepth = kHfRingWords / 4;   // hf_decode_kernel: a lane queues 2 * kHfQueueDepth varblock descriptors
JXL_LAYOUT int HfSlots(int sections) { return (sections + 3) & ~3; }   // lanes a task's arrays are laid out for
struct HfLds {
  size_t ring, descq, nzcol, tables;   // tables: the lanes' bytes alone
  JXL_LAYOUT explicit HfLds(int nslots) {
    ring = 0;
    descq = ring + (size_t)nslots * kHfRingWords * 4;
    nzcol = descq + (size_t)nslots * 2 * kHfQueueDepth * 4;
    tables = nzcol + (size_t)nslots * kNzColBytes;
  }
};
JXL_LAYOUT size_t HfLaneBytes(int nslots) { return HfLds(nslots).tables; }
JXL_LAYOUT size_t HfTablesEnd(size_t off, const CodeShape& s) { return CodeLds(off, s).end + kNnzCtxBytes; }
JXL_LAYOUT size_t HfTablesBytes(const CodeShape& s) { return CodeLdsBytes(s) + kNnzCtxBytes + kHfTailAllowance; }
// what the lane-stride heuristic takes for a workgroup's LDS: the tables (without the tail allowance) and four lanes
JXL_LAYOUT size_t HfEstimateBytes(const CodeShape& s) { return CodeLdsBytes(s) + kNnzCtxBytes + HfLaneBytes(kHfEstimateLanes); }

// ---- recon_tile_kernel (tile_kernels.hip): three coefficient tiles | the 8- and 16-point bases | per-cell tables | matrix-core tables
// The same for every launch.  csc holds pointers (8-byte aligned), the three basis tables are read in 16-byte pieces.
constexpr int kReconTileSide = 64;    // a tile is 64 x 64 samples, 8 x 8 cells
constexpr int kReconTilePitch = 65;   // floats per tile row in LDS (conflict-free column walks)
constexpr int kReconTileFloats = kReconTileSide * kReconTilePitch;
struct ReconTileLds {
  size_t cfc3;     // 3 tiles of f32: coefficients -> columns done -> pixels; team order Y, X, B
  size_t B816;     // 320 f32: IDCT bases of the two common sizes (N = 8 at 0, N = 16 at 64)
  size_t cscale;   // 64 f32, per cell: inv_global_scale / raw quant of its varblock
  size_t ci;       // 64 u32: cell info
  size_t cmeta;    // 64 u32: log2 of the stored pitch | transposed << 4
  size_t cnq;      // 64 u32: entries per channel of the cell's dequantisation table
  size_t cpre;     // 3 x 64 u32: exclusive prefix of the entry counts per team ...
  size_t cstart;   // 3 x 64 u32: ... and where each origin cell's entries start in the group's list
  size_t ctot;     // 4 u32: totals per team; [3]: the tile holds a 64-point varblock
  size_t csc;      // 64 pointers: scan list of the cell's quant table
  size_t t32_lo;   // 128 float4: k-contiguous 32-point basis, first / second four k-steps of lane (n, q) = [n * 4 + q]
  size_t t32_hi;   // 128 float4
  size_t t64;      // 4 x 256 float4: the 64-point basis, quarter j of lane (n, q) = [j * 256 + n * 4 + q]
  size_t end;
  JXL_LAYOUT constexpr ReconTileLds()
      : cfc3(0), B816(cfc3 + 3 * (size_t)kReconTileFloats * 4), cscale(B816 + 320 * 4), ci(cscale + 64 * 4), cmeta(ci + 64 * 4), cnq(cmeta + 64 * 4),
        cpre(cnq + 64 * 4), cstart(cpre + 3 * 64 * 4), ctot(cstart + 3 * 64 * 4), csc(ctot + 4 * 4), t32_lo(csc + 64 * 8), t32_hi(t32_lo + 128 * 16),
        t64(t32_hi + 128 * 16), end(t64 + 4 * 256 * 16) {}
};
static_assert(ReconTileLds().csc % 8 == 0 && ReconTileLds().t32_lo % 16 == 0 && ReconTileLds().t32_hi % 16 == 0 && ReconTileLds().t64 % 16 == 0,
              "the pointers and the 16-byte pieces are aligned");
static_assert(ReconTileLds().end == 74768, "three tiles, the small bases, the per-cell tables and 20 KB of matrix-core tables");

}  // namespace jxlhip
