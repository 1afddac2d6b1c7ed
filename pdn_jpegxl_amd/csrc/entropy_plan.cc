// The entropy stage's launch plan (entropy_plan.h).  Host arithmetic only: this file makes no HIP call.
#include "entropy_plan.h"
#include <algorithm>
#include "../../include/jxlfiletypeio.h"

namespace jxlhip {

// (the vectors' sizes rather than num_hist: a code that has not been read yet - the HF code of a one-section frame before its LF
// pre-pass - has no tables)
CodeShape ShapeOf(const HostCode& hc) {
  return CodeShape{(uint32_t)hc.cfg.size(), hc.log_alpha, (uint32_t)hc.ctx_map.size(), hc.use_prefix || hc.alias.empty()};
}

EntropyPlan PlanEntropy(const std::vector<ParsedFrame>& frames, const std::vector<int>& parse_status, const EntropyPlanOptions& opt) {
  EntropyPlan P;
  const int n = (int)frames.size();
  const bool ds = opt.downscale == 8;
  const int band_first_row = opt.band_first_row, band_rows = opt.band_rows;
  auto ok = [&](int i) { return parse_status[i] == DecoderStatus_Ok; };
  auto lossy = [&](int i) { return ok(i) && frames[i].encoding == 0; };
  P.frames.assign((size_t)n, FramePlan());
  // every pass after the first of a progressive frame is an image record of its own, after the batch's n (dev_types.h: next_pass)
  for (int i = 0; i < n; i++) {
    P.frames[i].first_extra = n + P.n_extra;
    if (lossy(i)) P.n_extra += (int)frames[i].extra_passes.size();
  }
  int total_lf = 0, total_groups = 0;
  for (int i = 0; i < n; i++) {
    if (!ok(i)) continue;
    const ParsedFrame& f = frames[i];
    FramePlan& r = P.frames[i];
    r.decoded = true;
    // band: group rows [b0, b1) are output; one more row each side is decoded for the loop-filter halo
    int b0 = 0, b1 = (int)f.yg;
    if (band_rows > 0 && f.encoding == 0) { b0 = std::min<int>(band_first_row, (int)f.yg); b1 = std::min<int>(b0 + band_rows, (int)f.yg); }
    r.dec_gy0 = std::max(0, b0 - 1); r.dec_gy1 = std::min<int>((int)f.yg, b1 + 1);
    r.band_y0 = std::min<int>(b0 * kGroupDim, (int)f.ysize); r.band_y1 = std::min<int>(b1 * kGroupDim, (int)f.ysize);
    if (f.encoding != 0) continue;
    // (a reduced-size decode reads the HF tokens only for what follows them in a section - the alpha channel - and keeps no coefficients
    // of an opaque frame)
    r.hf = !ds || f.alpha_index >= 0;
    // LF groups that intersect the decoded group rows (8 group rows per LF group row); HF groups of the decoded rows; alpha of the band
    const uint32_t lfy0 = (uint32_t)r.dec_gy0 / 8, lfy1 = ((uint32_t)r.dec_gy1 + 7) / 8;
    r.lf0 = lfy0 * f.xlf; r.lf1 = std::min<uint32_t>(f.nlf, lfy1 * f.xlf);
    r.hf0 = (uint32_t)r.dec_gy0 * f.xg; r.hf1 = (uint32_t)r.dec_gy1 * f.xg;
    r.alpha0 = (uint32_t)(r.band_y0 / kGroupDim) * f.xg; r.alpha1 = (uint32_t)((r.band_y1 + kGroupDim - 1) / kGroupDim) * f.xg;
    // sections this call decodes (a band: its group rows + one each side, the LF groups they touch): what the launch shapes go by
    total_lf += (int)(r.lf1 - r.lf0);
    if (r.hf) total_groups += (int)(r.hf1 - r.hf0) * (int)f.num_passes;
  }
  // Modular frames whose MA tree looks at decoded neighbours take the generic per-lane path: give it LDS row buffers (groups of up to
  // 256 columns); with the weighted predictor its per-sample state goes to LDS as well, which limits a workgroup to 8 sections
  int mod_lanes = 64, mod_rb = 0, mod_wp_lds = 0;
  size_t total_mod_sections = 0;
  for (int i = 0; i < n; i++) {
    if (!ok(i) || frames[i].encoding != 1) continue;
    if (!frames[i].tree_row_static && frames[i].group_dim <= 256) mod_rb = 256;
    if (frames[i].tree_uses_wp && frames[i].group_dim <= 256) { mod_wp_lds = 1; mod_lanes = 8; }
    total_mod_sections += frames[i].single ? 1 : 1 + (size_t)frames[i].nlf + frames[i].ng;
  }
  if (!mod_rb) { mod_wp_lds = 0; mod_lanes = 64; }
  // few sections (one frame, a small batch): one section per wavefront - no divergence between sections, and row-static channels
  // decode on the scalar unit from per-residue tables (see the LF launch below)
  if (total_mod_sections <= 512 && !opt.mod_lanes64) mod_lanes = 1;
  P.mod_lanes = mod_lanes; P.mod_rb = mod_rb; P.mod_wp_lds = mod_wp_lds;
  // Small launches get the Modular code's per-residue tables (the alias tables spelled out for each of the 4096 state residues,
  // 16 KB per cluster, codes of up to 8 clusters): one-section wavefronts read them through the scalar cache (RowScalar).  Measured
  // against a copy in LDS (one 4K frame): lf_ans 20.2 -> 18.8 ms, alpha_ans 5.7 -> 5.1 ms, and no LDS spent on them.
  bool global_direct = false;
  if (!opt.no_direct) {
    int pre_lf = 0;
    for (int i = 0; i < n; i++) if (lossy(i)) pre_lf += (int)frames[i].nlf;
    global_direct = n <= 64 && pre_lf <= 1024 && total_mod_sections <= 512;
  }
  P.global_direct = global_direct;
  // Lane mapping of the HF kernel: one wavefront per section while every workgroup of the launch can be resident at once
  // (the kernel is latency-bound, a second round of workgroups doubles its time); otherwise pack more sections per wavefront.
  int lane_stride = 64;
  int hf_wg_capacity = 256 * 8;   // workgroups of the HF kernel that can be resident at once (by the LDS of the widest tables)
  if (opt.lane_stride_override > 0) lane_stride = opt.lane_stride_override;
  else {
    size_t lds_est = 0;
    for (int i = 0; i < n; i++)
      if (lossy(i)) lds_est = std::max(lds_est, HfEstimateBytes(ShapeOf(frames[i].acode)));
    const int wg_per_cu = lds_est ? (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / lds_est)) : 8;
    const int capacity = 256 * wg_per_cu;   // resident 256-thread workgroups on the chip
    hf_wg_capacity = capacity;
    while (lane_stride > 1 && (total_groups + (256 / lane_stride) - 1) / (256 / lane_stride) > capacity) lane_stride >>= 1;
    // measured (MI355X, 4K frames, batch 384): once a batch holds thousands of sections, 32 sections per wavefront
    // (half-filled wavefronts, five per image instead of three) is the best trade between instruction efficiency and wavefronts
    // in flight: hf_decode 72 ms (stride 1) / 61 ms (stride 2) / 87 ms (stride 4)
    if (total_groups >= 8192) lane_stride = 2;
    if (opt.hf_stride_override > 0) lane_stride = opt.hf_stride_override;
  }
  P.lane_stride = lane_stride;
  // Workgroup width of the HF kernel: four wavefronts, or up to eight when the sections are spread thinly over the lanes and one
  // image's sections would otherwise need a second workgroup (each workgroup stages the image's ~50 KB of tables in LDS).
  int hf_waves = 4;
  {
    int max_ng = 0;
    for (int i = 0; i < n; i++)
      if (lossy(i)) max_ng = std::max<int>(max_ng, (int)frames[i].ng);
    const int per_wave = 64 / lane_stride;
    const int need = (max_ng + per_wave - 1) / per_wave;
    if (need > 4 && lane_stride <= 8) hf_waves = std::min(8, need);
    if (lane_stride == 64 && !opt.hf_waves8) {
      // One section per wavefront: its token loop runs on the scalar unit, and a CU has ONE scalar unit - eight such wavefronts in
      // a workgroup share it (measured: hf_decode of one 4K frame 12.5 ms with 17 workgroups of 8 wavefronts).  Spread the sections
      // over as many workgroups as can be resident at once, one wavefront each if they all fit.
      hf_waves = 1;
      while (hf_waves < 8 && (total_groups + hf_waves - 1) / hf_waves > hf_wg_capacity) hf_waves *= 2;
    }
  }
  P.hf_waves = hf_waves;
  const int per_wg = hf_waves * (64 / lane_stride);
  // Sections per workgroup, per image: the HF kernel's LDS is the image's code tables (30 .. 60 KB: they double with the alias-table
  // width) plus 288 B per lane, and a launch has ONE LDS size.  Sized by the batch-wide maximum, a single image with wide tables
  // pushed every workgroup from two per CU to one (hf_decode 30 -> 58 ms at batch 384); instead every image gets as many lanes per
  // workgroup as fit beside ITS tables in the budget (whole wavefronts; images with wide tables use more, smaller workgroups).
  // The budget (half a CU's LDS) was re-measured in round 3 against 96 / 112 / 128 KB (one workgroup per 4K frame, one copy of its
  // tables): those won 6 % of the pipelined step while the fused filter kernel held 252 registers, and nothing since it holds 122
  // (profiles/r03_experiment_hf_lds_budget.txt, r03_experiment_pairs_balance.txt); alone, the HF kernel is 36 ms with 80 KB and 65 ms
  // with 112 KB (two rounds of workgroups), so 80 KB it stays.
  auto hf_table_bytes = [](const ParsedFrame& f) {   // the widest of the frame's passes
    size_t b = HfTablesBytes(ShapeOf(f.acode));
    for (auto& ep : f.extra_passes) b = std::max(b, HfTablesBytes(ShapeOf(ep.acode)));
    return b;
  };
  size_t kHfLdsTarget = 80 * 1024;
  if (opt.hf_lds_kb >= 32 && opt.hf_lds_kb <= 160) kHfLdsTarget = (size_t)opt.hf_lds_kb * 1024;   // experiment knob
  auto hf_per_wg = [&](const ParsedFrame& f) {
    // the fewest workgroups whose (tables + lanes) fit the budget, the image's sections spread evenly over them: every workgroup
    // carries a copy of the tables, so a small last workgroup (64 + 64 + 7 sections) costs a full LDS slot for a few lanes
    const int per_wave = 64 / lane_stride;
    const size_t tab = hf_table_bytes(f);
    const int ng = std::max(1, (int)f.ng);
    for (int nwg = 1; nwg <= ng; nwg++) {
      const int lanes = (((ng + nwg - 1) / nwg) + per_wave - 1) / per_wave * per_wave;
      if (lanes <= per_wg && tab + HfLaneBytes(lanes) <= kHfLdsTarget) return lanes;
      if (lanes <= per_wave) break;
    }
    return per_wave;
  };
  for (int i = 0; i < n; i++)
    if (lossy(i)) { P.frames[i].hf_table_bytes = hf_table_bytes(frames[i]); P.frames[i].hf_per_wg = hf_per_wg(frames[i]); }
  // Lane mapping of the alpha phase-A kernel (one wavefront per workgroup, sections of one image per wavefront): spread the
  // sections over as many wavefronts as the chip holds in one round, then pack.
  int alpha_stride = 64;
  if (opt.lane_stride_override > 0) alpha_stride = opt.lane_stride_override;
  else {
    int alpha_sections = 0;
    for (int i = 0; i < n; i++)
      if (lossy(i) && frames[i].alpha_index >= 0) alpha_sections += (int)(P.frames[i].alpha1 - P.frames[i].alpha0);   // a band decodes the alpha of its own group rows only
    // Two good shapes and a bad middle (measured, 4K frames): one section per wavefront on the scalar unit (5 ms for 135 sections,
    // degrading gently while a CU holds a dozen such wavefronts) and 32 sections per wavefront on the vector unit (12 ms for 8640
    // sections); 2 ... 16 sections per wavefront pay the vector chain for a few lanes (21 ms for 2160 sections at 2 per wavefront).
    if (global_direct && !opt.alpha_old_shapes) alpha_stride = alpha_sections > 3072 ? 2 : 64;
    else while (alpha_stride > 1 && alpha_sections / (64 / alpha_stride) > 256 * 8) alpha_stride >>= 1;
    if (alpha_sections >= 8192) alpha_stride = 2;   // measured: alpha_ans 27.8 ms (stride 1) / 22.5 (2) / 26.4 (4) at batch 384
    if (opt.alpha_stride > 0) alpha_stride = opt.alpha_stride;   // experiment knob
  }
  P.alpha_stride = alpha_stride;
  const int per_alpha_wg = 64 / alpha_stride;
  P.per_alpha_wg = per_alpha_wg;
  // LF groups per wavefront of the LF phase-A kernel.  Measured on MI355X: the 64 LF groups of a 16384^2 frame in ONE wavefront (every
  // lane walking its own divergent stream) took 68 ms against 33 ms for the four of a 4K frame; one group per wavefront is no faster
  // for a single frame and much slower for a batch (384 frames: 44 -> 67 ms, four times the wavefronts for the same tokens).  So: four
  // per wavefront, more only when a batch brings tens of thousands of LF groups.
  // LF sections per wavefront: one while the batch is small (the wavefront's recurrence then runs on the scalar unit: lower latency),
  // four for large batches (fewer wavefronts and table copies for the same latency-bound time), more only for huge ones
  int lf_per_wave = total_lf <= 256 ? 1 : 4;
  while (lf_per_wave < 64 && total_lf / lf_per_wave > 4096) lf_per_wave *= 2;
  if (opt.lf_per_wave > 0) lf_per_wave = std::min(64, opt.lf_per_wave);   // experiment knob
  P.lf_per_wave = lf_per_wave;
  // wavefronts that decode one section run their row loops on the scalar unit from the per-residue tables
  // (measured at batch 384: LF sections as four such wavefronts per workgroup - 135.7 ms per batch against 125.1 with four lanes of
  // one wavefront: large batches keep the lane layout, the scalar path is for small ones)
  P.direct_lf = global_direct && lf_per_wave == 1; P.direct_alpha = global_direct && per_alpha_wg == 1; P.direct_mod = global_direct && mod_lanes == 1;
  // the lean forms of the LF / alpha kernels (no per-sample Modular path compiled in: two thirds of the registers) when no lossy frame
  // of the batch can take that path: row-static MA tree, standard predictors, plain ANS codes
  for (int i = 0; i < n; i++)
    if (lossy(i) && (!frames[i].tree_row_static || frames[i].tree_uses_wp || frames[i].mcode.use_prefix || frames[i].mcode.lz77)) P.lean_mod = false;
  // ---- task tables and the launches' LDS
  const bool mod_uniform = ModularUniform(mod_lanes, mod_rb);
  for (int i = 0; i < n; i++) {
    if (!ok(i)) continue;
    const ParsedFrame& f = frames[i];
    const FramePlan& r = P.frames[i];
    const CodeShape mshape = ShapeOf(f.mcode);
    if (f.encoding == 1) {
      P.mod.lds = std::max(P.mod.lds, ModularLdsBytes(mod_lanes, mod_rb, mod_wp_lds, mod_uniform, f.tree.size(), mshape));
      const uint32_t nsec = 1 + f.nlf + f.ng;
      P.max_mod_groups = std::max<int>(P.max_mod_groups, (int)nsec);
      P.max_mod_coded = std::max<int>(P.max_mod_coded, (int)f.mod_coded.size());
      if (f.single) P.mod_tasks.push_back(SectionTask{i, 0, 1, 0});   // one bit stream: one lane walks all three sections
      else for (uint32_t g = 0; g < nsec; g += mod_lanes) P.mod_tasks.push_back(SectionTask{i, (int32_t)g, (int32_t)std::min<uint32_t>(mod_lanes, nsec - g), 0});
      continue;
    }
    P.lf.lds = std::max(P.lf.lds, SlotsLdsBytes(lf_per_wave, f.tree.size(), mshape));
    // (the lane path finishes alpha groups in one pass: every lane keeps its group's previous row behind the tables)
    P.alpha.lds = std::max(P.alpha.lds, SlotsLdsBytes(per_alpha_wg, f.tree.size(), mshape) + (P.direct_alpha ? 0 : AlphaRowsLdsBytes(per_alpha_wg)));
    for (uint32_t g = r.lf0; g < r.lf1; g++) P.lf_finish_tasks.push_back(SectionTask{i, (int32_t)g, 1, 0});
    for (uint32_t g = r.lf0; g < r.lf1; g += lf_per_wave)
      P.lf_ans_tasks.push_back(SectionTask{i, (int32_t)g, (int32_t)std::min<uint32_t>((uint32_t)lf_per_wave, r.lf1 - g), 0});
    const uint32_t hg0 = r.hf0, hg1 = r.hf1;
    const uint32_t pw = (uint32_t)r.hf_per_wg;
    for (uint32_t pass = 0; pass < (r.hf ? f.num_passes : 0u); pass++) {
      // Sections go to lanes in order of their byte size (the TOC has it), largest first: a wavefront runs until its longest
      // section ends, so lanes of similar length finish together (the sum over wavefronts of their longest lane - the
      // wave-instructions of the launch - nearly halves for 4K frames, whose sections spread 1 : 2.2 around the mean), and the
      // longest sections start first.  Slot j of the (image, pass) decodes group hf_order[j]; tasks index slots.
      P.hf_orders.push_back(EntropyPlan::HfOrder{i, (int)pass, std::vector<uint32_t>(hg1 - hg0)});
      std::vector<uint32_t>& order = P.hf_orders.back().order;
      const size_t sec0 = f.single ? 0 : 2 + (size_t)f.nlf + (size_t)pass * f.ng;
      for (uint32_t g = hg0; g < hg1; g++) order[g - hg0] = g;
      if (!f.single && !opt.no_hf_sort)   // (experiment knob: measured effect of the order, profiles/r03_hf_sort_ab.txt)
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return f.sec_size[sec0 + a] > f.sec_size[sec0 + b]; });
      for (uint32_t j = 0; j < hg1 - hg0; j += pw) {
        const uint32_t cnt = std::min<uint32_t>(pw, hg1 - hg0 - j);
        P.pass_tasks.push_back(SectionTask{pass ? r.first_extra + (int)pass - 1 : i, (int32_t)j, (int32_t)cnt, 0});
        const size_t lanes = HfLaneBytes(HfSlots((int)cnt));   // the kernel lays its per-lane arrays out for the task's lanes
        P.hf.lds = std::max(P.hf.lds, r.hf_table_bytes + lanes);
        P.lds_hf_lanes = std::max(P.lds_hf_lanes, lanes);
      }
    }
    if (f.alpha_index >= 0)
      for (uint32_t g = r.alpha0; g < r.alpha1; g += per_alpha_wg)
        P.alpha_tasks.push_back(SectionTask{i, (int32_t)g, (int32_t)std::min<uint32_t>(per_alpha_wg, r.alpha1 - g), 0});
  }
  // experiment knobs: code tables of the entropy kernels read from global memory (L1 / L2) instead of LDS copies
  P.hf.global = P.hf.lds > kLdsMax || opt.hf_global;
  P.alpha.global = P.alpha.lds > kLdsMax || opt.alpha_global;
  P.lf.global = P.lf.lds > kLdsMax || opt.lf_global;
  P.mod.global = P.mod.lds > kLdsMax;
  return P;
}

}  // namespace jxlhip
