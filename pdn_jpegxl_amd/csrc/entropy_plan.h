// The launch plan of a batch's entropy stage: which sections each call decodes, how they map to lanes and workgroups, the task tables
// and the dynamic LDS of the four serial kernels (lds_layout.h).  Pure arithmetic on parsed frames and options: no HIP calls, so the
// CPU suite checks it (tests/test_entropy_plan.py).  JxlHipDecoder::Decode calls PlanEntropy once, after its refusals.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "host_parse.h"
#include "lds_layout.h"

namespace jxlhip {

struct EntropyPlanOptions {
  int band_first_row = 0, band_rows = 0;   // band-restricted decode: 0 rows = whole frame
  int downscale = 1;
  int lane_stride_override = 0, hf_stride_override = 0;
  bool no_direct = false, mod_lanes64 = false;
  // values of the experiment knobs (a library built with -DJXLHIP_EXPERIMENTS reads them from the environment; 0 / false: not set)
  bool hf_waves8 = false, alpha_old_shapes = false, no_hf_sort = false;
  bool hf_global = false, alpha_global = false, lf_global = false;   // code tables read from global memory instead of LDS copies
  int hf_lds_kb = 0, alpha_stride = 0, lf_per_wave = 0;
};

// What one call decodes of a frame.  Group rows [band_y0, band_y1) / kGroupDim are output; one more row each side is decoded for the
// loop-filter halo, with the LF groups those rows touch; alpha is decoded for the band's own rows only.
struct FramePlan {
  bool decoded = false;   // false: the frame failed to parse or was refused; it contributes nothing
  int dec_gy0 = 0, dec_gy1 = 0, band_y0 = 0, band_y1 = 0;
  uint32_t lf0 = 0, lf1 = 0, hf0 = 0, hf1 = 0, alpha0 = 0, alpha1 = 0;   // LF groups / HF groups / alpha groups [first, end)
  bool hf = false;             // does hf_decode_kernel run for this frame?  (reduced size: only to find the alpha stream)
  int first_extra = 0;         // image record of the frame's second pass (records of further passes follow the batch's frames)
  int hf_per_wg = 0;           // HF sections per workgroup
  size_t hf_table_bytes = 0;   // the widest of the frame's passes
};

struct EntropyLaunch {
  size_t lds = 0;        // tables + lanes of the largest workgroup
  bool global = false;   // the variant that keeps its tables in global memory is launched (lds > kLdsMax, or a knob)
  size_t Bytes() const { return global ? 0 : lds; }   // what the Launch* wrappers take
};

struct EntropyPlan {
  std::vector<FramePlan> frames;
  int n_extra = 0;   // image records of later passes
  bool global_direct = false, lean_mod = true;
  int lane_stride = 64, hf_waves = 4, alpha_stride = 64, per_alpha_wg = 1, lf_per_wave = 1;
  int mod_lanes = 64, mod_rb = 0, mod_wp_lds = 0;
  int direct_lf = 0, direct_alpha = 0, direct_mod = 0;
  EntropyLaunch lf, hf, alpha, mod;
  size_t lds_hf_lanes = 0;   // the most lanes of an HF workgroup (global-table variant)
  std::vector<SectionTask> lf_finish_tasks, lf_ans_tasks, pass_tasks, alpha_tasks, mod_tasks;
  // slot j of an (image, pass) decodes group order[j]; pass tasks index slots
  struct HfOrder { int image, pass; std::vector<uint32_t> order; };
  std::vector<HfOrder> hf_orders;
  int max_mod_groups = 1, max_mod_coded = 1;
};

CodeShape ShapeOf(const HostCode& hc);
EntropyPlan PlanEntropy(const std::vector<ParsedFrame>& frames, const std::vector<int>& parse_status, const EntropyPlanOptions& opt);

}  // namespace jxlhip
