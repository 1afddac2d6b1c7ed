// The layout of a decode batch (batch_layout.h): every buffer is sized, typed and assigned in one statement of BuildBatch.
#include "batch_layout.h"
#include "varblock_rules.h"
#include <cmath>
#include "../../include/jxlfiletypeio.h"

namespace jxlhip {

// Order bucket of a quant table (every strategy of a quant table shares one bucket).
static int OrderBucketOfQuantTable(int q) {
  for (int s = 0; s < kNumStrategies; s++) if ((int)StrategyQuantTable(s) == q) return (int)StrategyOrderBucket(s);
  return 0;
}

void BuildScanList(int q, const std::vector<uint16_t> (*custom)[3], U32x2* out, const std::vector<float>* custom_dq) {
  const StaticTables& st = GetStaticTables();
  const int o = OrderBucketOfQuantTable(q);
  const std::vector<float>& dq = (custom_dq && custom_dq->size() == st.dq[q].size()) ? *custom_dq : st.dq[q];
  const size_t n = st.dq[q].size() / 3;
  for (int c = 0; c < 3; c++) {
    const std::vector<uint16_t>& ord = (custom && !custom[o][c].empty()) ? custom[o][c] : st.natural_order[o];
    for (size_t k = 0; k < n; k++) {
      const uint32_t p = k < ord.size() ? ord[k] : 0u;
      uint32_t wb;
      const float w = dq[(size_t)c * n + (p < n ? p : 0)];
      memcpy(&wb, &w, 4);
      out[(size_t)c * n + k] = U32x2{p, wb};
    }
  }
}

void PackCode(const HostCode& hc, Region& blob, DevCode& dc) {
  memset(&dc, 0, sizeof(dc));
  dc.ctx_map = blob.Put(hc.ctx_map.data(), hc.ctx_map.size());
  dc.cfg = blob.Fill<uint32_t>(hc.cfg.size(), [&](uint32_t* cfg) {
    for (size_t k = 0; k < hc.cfg.size(); k++) {
      cfg[k] = hc.cfg[k].split | hc.cfg[k].msb << 4 | hc.cfg[k].lsb << 8;
      if (hc.use_prefix) {   // one-symbol prefix codes read no bits
        if (hc.prefix[k].single >= 0) cfg[k] |= 1u << 12 | (uint32_t)hc.prefix[k].single << 16;
        continue;
      }
      // single-symbol clusters: decoding never changes the ANS state nor reads bits (alias special form)
      const uint64_t e0 = hc.alias[k << hc.log_alpha];
      const uint32_t x0 = (uint32_t)e0, y0 = (uint32_t)(e0 >> 32);
      if ((x0 >> 16) == 0 && (y0 >> 16) == 4096) cfg[k] |= 1u << 12 | ((x0 >> 8) & 0xFF) << 16;
    }
  });
  dc.alias = blob.Put(hc.alias.data(), hc.alias.size());
  if (hc.use_prefix) {   // counts per length, symbol offsets, symbols sorted by code
    size_t total = 0;
    for (auto& pc : hc.prefix) total += pc.sorted.size();
    dc.pfx_count = blob.Fill<uint16_t>(16 * hc.prefix.size(), [&](uint16_t* h) {
      for (size_t k = 0; k < hc.prefix.size(); k++) memcpy(h + 16 * k, hc.prefix[k].count, 32);
    });
    dc.pfx_off = blob.Fill<uint32_t>(hc.prefix.size(), [&](uint32_t* h) {
      uint32_t at = 0;
      for (size_t k = 0; k < hc.prefix.size(); k++) { h[k] = at; at += (uint32_t)hc.prefix[k].sorted.size(); }
    });
    dc.pfx_sorted = blob.Fill<uint16_t>(std::max<size_t>(1, total), [&](uint16_t* h) {
      for (auto& pc : hc.prefix) { if (!pc.sorted.empty()) memcpy(h, pc.sorted.data(), 2 * pc.sorted.size()); h += pc.sorted.size(); }
    });
  }
  if (hc.lz77) {
    dc.lz_min_symbol = hc.lz_min_symbol; dc.lz_min_length = hc.lz_min_length;
    dc.lz_len_cfg = hc.lz_len.split | hc.lz_len.msb << 4 | hc.lz_len.lsb << 8;
    dc.lz_dist_cluster = hc.ctx_map.back();
  }
  dc.num_ctx = (uint32_t)hc.ctx_map.size();
  dc.num_clusters = hc.num_hist;
  dc.log_alpha = hc.log_alpha;
  dc.slow = (hc.use_prefix ? 1u : 0u) | (hc.lz77 ? 2u : 0u);
}

// The alias tables of an ANS code spelled out per state residue (DevCode::direct).
static void BuildDirectTable(const HostCode& hc, uint32_t* dt) {
  const uint32_t la = hc.log_alpha, le = 12 - la;
  for (uint32_t r = 0; r < (hc.num_hist << 12); r++) {
    const uint32_t cl = r >> 12, res = r & 0xFFF, i = res >> le, pos = res & ((1u << le) - 1);
    const uint64_t e = hc.alias[(cl << la) + i];
    const uint32_t x = (uint32_t)e, y = (uint32_t)(e >> 32);
    const bool g = pos >= (x & 0xFF);
    const uint32_t sym = g ? ((x >> 8) & 0xFF) : i, o = g ? (y & 0xFFFF) + pos : pos, freq = g ? ((x >> 16) ^ (y >> 16)) : (x >> 16);
    dt[r] = ((freq - 1) & 0xFFF) | ((o & 0xFFF) << 12) | (sym << 24);
  }
}

PatchTables BuildPatchTables(const std::vector<ParsedFrame>& frames, const std::vector<int>& parse_status, const std::vector<Composite>& comps) {
  PatchTables T;
  for (const Composite& c : comps)
    for (int j = 0; j < c.count; j++) {
      const int i = c.first + j;
      const ParsedFrame& f = frames[i];
      if (parse_status[i] != DecoderStatus_Ok || f.patch_pos.empty()) continue;
      const int pf = (int)T.image.size(), ref0 = (int)T.refs.size(), pos0 = (int)T.pos.size();
      T.image.push_back(i);
      T.first.push_back(c.first);
      for (auto& rr : f.patch_refs) {
        PatchRef r;
        memset(&r, 0, sizeof(r));
        r.w = (int32_t)rr.w; r.h = (int32_t)rr.h;
        T.refs.push_back(r);
      }
      const int tx = (int)((f.xsize + kPatchTile - 1) / kPatchTile), ty = (int)((f.ysize + kPatchTile - 1) / kPatchTile);
      std::vector<std::vector<int32_t>> lists((size_t)tx * ty);
      std::vector<PatchTile> box((size_t)tx * ty);
      for (size_t k = 0; k < f.patch_pos.size(); k++) {
        const ParsedFrame::PatchPlace& q = f.patch_pos[k];
        PatchPos p;
        memset(&p, 0, sizeof(p));
        p.x = (int32_t)q.x; p.y = (int32_t)q.y; p.ref = ref0 + (int32_t)q.ref;
        for (int g = 0; g < 2; g++) { p.mode[g] = q.mode[g]; p.clamp[g] = q.clamp[g]; }
        T.pos.push_back(p);
        if (q.mode[0] == 0 && (f.alpha_index < 0 || q.mode[1] == 0)) continue;   // None everywhere: no pixel changes
        const int x1 = p.x + (int)f.patch_refs[q.ref].w, y1 = p.y + (int)f.patch_refs[q.ref].h;
        for (int b = p.y / kPatchTile; b * kPatchTile < y1; b++)
          for (int a = p.x / kPatchTile; a * kPatchTile < x1; a++) {
            const size_t t = (size_t)b * tx + a;
            PatchTile& bx = box[t];
            const int cx0 = std::max(p.x, a * kPatchTile), cy0 = std::max(p.y, b * kPatchTile);
            const int cx1 = std::min(x1, (a + 1) * kPatchTile), cy1 = std::min(y1, (b + 1) * kPatchTile);
            if (lists[t].empty()) { bx.x0 = cx0; bx.y0 = cy0; bx.x1 = cx1; bx.y1 = cy1; }
            else { bx.x0 = std::min(bx.x0, cx0); bx.y0 = std::min(bx.y0, cy0); bx.x1 = std::max(bx.x1, cx1); bx.y1 = std::max(bx.y1, cy1); }
            lists[t].push_back(pos0 + (int32_t)k);
          }
      }
      for (size_t t = 0; t < lists.size(); t++) {
        if (lists[t].empty()) continue;   // tiles without patches get no workgroup
        PatchTile tl = box[t];
        tl.frame = pf; tl.first = (int32_t)T.list.size(); tl.count = (int32_t)lists[t].size(); tl.pad = 0;
        T.tiles.push_back(tl);
        T.list.insert(T.list.end(), lists[t].begin(), lists[t].end());
      }
    }
  return T;
}

void BuildBatch(const BatchInput& in, BatchRegions& R, BatchOutput& out) {
  const std::vector<ParsedFrame>& frames = *in.frames;
  const std::vector<int>& parse_status = *in.parse_status;
  const EntropyPlan& plan = *in.plan;
  Region &blob = R.blob, &wz = R.zero, &ws = R.ws, &px = R.pix;
  const int n = (int)frames.size();
  const bool ds = in.ds;
  auto decoded = [&](int i) { return parse_status[i] == DecoderStatus_Ok; };
  std::vector<DevImage>& imgs = out.imgs;
  imgs.resize((size_t)n + plan.n_extra);   // every pass after the first of a progressive frame is an image record of its own
  if (!imgs.empty()) memset(imgs.data(), 0, sizeof(DevImage) * imgs.size());   // (failed or refused images stay zeroed: ng = 0)
  out.status_off.assign(n, 0);
  out.d_imgs = blob.Array<DevImage>(imgs.size());
  // the images' status words (64 B each) lie side by side: ONE copy brings them back (a copy per image was 384 five-microsecond copy
  // kernels at the end of the pixel stream - 2 ms of the step - and as many API calls)
  out.status_base = wz.Array<uint32_t>((size_t)std::max(1, n) * 16);
  // The float planes between reconstruction and the loop filters (24 B/px) are only alive while a frame is in the pixel stages:
  // frames go through those stages in chunks that share pixel_chunk sets of planes, so the batch size is bounded by the
  // entropy-stage state (12 B/px of coefficients), not by 36 B/px.  (A third set: the loop-filter ping-pong planes, which double as the
  // dense coefficient planes of the generic path.)  Frames with synthetic noise: three more planes per chunk slot for the convolved
  // noise the output phase adds (12 B/px, only when a frame of the batch has noise); the random planes they are made from live in tmp.
  // A reduced-size decode has no reconstruction and no filters: no pixel planes.
  const int pixel_chunk = out.pixel_chunk = in.debug_taps ? std::max(1, n) : std::min(std::max(1, n), in.pixel_chunk_cap);
  size_t chunk_pix = 0, noise_pix = 0;   // padded pixels of the largest VarDCT frame / pixels of the largest frame with noise
  for (int i = 0; i < n; i++) {
    if (!decoded(i) || ds) continue;
    if (frames[i].encoding == 0) chunk_pix = std::max(chunk_pix, (size_t)frames[i].w8 * frames[i].h8 * 64);
    if (frames[i].has_noise) noise_pix = std::max(noise_pix, (size_t)frames[i].xsize * frames[i].ysize);
  }
  struct ChunkPlanes { float *tmp, *xyb, *noise; int32_t* coef; };
  std::vector<ChunkPlanes> chunk((size_t)pixel_chunk * 3, ChunkPlanes{nullptr, nullptr, nullptr, nullptr});
  if (chunk_pix)
    for (ChunkPlanes& p : chunk) { p.tmp = px.Array<float>(chunk_pix); p.xyb = px.Array<float>(chunk_pix); p.coef = px.Array<int32_t>(chunk_pix); }
  if (noise_pix)
    for (ChunkPlanes& p : chunk) p.noise = px.Array<float>(noise_pix);
  // slot j of an (image, pass) decodes group hf_order[j]: the plan's orders by image record
  std::vector<const std::vector<uint32_t>*> order_of(imgs.size(), nullptr);
  for (const EntropyPlan::HfOrder& o : plan.hf_orders) order_of[o.pass ? (size_t)plan.frames[o.image].first_extra + o.pass - 1 : (size_t)o.image] = &o.order;
  auto put_order = [&](size_t rec, uint32_t ng) -> const uint32_t* {
    const std::vector<uint32_t>* o = order_of[rec];
    const uint32_t* p = blob.Put(o ? o->data() : nullptr, o ? o->size() : 0, std::max<uint32_t>(1, ng));
    return o ? p : nullptr;
  };
  // a frame's own scan list of quant table q (its own coefficient orders or dequantisation weights), or the library's
  auto scan_list = [&](int q, const std::vector<uint16_t> (*custom)[3], const std::vector<float>* dq) -> const U32x2* {
    const int o = OrderBucketOfQuantTable(q);
    if (!dq && custom[o][0].empty() && custom[o][1].empty() && custom[o][2].empty()) return in.d_scan[q];
    return blob.Fill<U32x2>(3 * (size_t)in.dq_n[q], [&](U32x2* h) { BuildScanList(q, custom, h, dq); });
  };
  // a codestream uploaded from the host: once per file (every frame of a layered file points into the same bytes)
  std::vector<const uint8_t*> file_cs((size_t)in.nfiles, nullptr);
  std::vector<uint8_t> file_cs_put((size_t)in.nfiles, 0);
  for (int i = 0; i < n; i++) {
    if (!decoded(i)) continue;
    const ParsedFrame& f = frames[i];
    const FramePlan& fp = plan.frames[i];
    DevImage& d = imgs[i];
    const size_t cells = (size_t)f.w8 * f.h8, tiles = (size_t)((f.w8 + 7) / 8) * ((f.h8 + 7) / 8), pixels = (size_t)f.xsize * f.ysize;
    d.w = f.xsize; d.h = f.ysize; d.w8 = f.w8; d.h8 = f.h8; d.wp = f.w8 * 8; d.hp = f.h8 * 8;
    d.wt = (f.w8 + 7) / 8; d.ht = (f.h8 + 7) / 8;
    d.xg = f.xg; d.yg = f.yg; d.ng = f.ng; d.xlf = f.xlf; d.ylf = f.ylf; d.nlf = f.nlf;
    d.ncolor = f.ncolor; d.has_alpha = f.alpha_index >= 0; d.nch_out = d.ncolor + d.has_alpha;
    d.sample_bits = (int32_t)f.bits; d.sample_exp = (int32_t)f.exp_bits;
    d.alpha_bits = d.has_alpha ? (int32_t)f.ec[f.alpha_index].bits : 8; d.alpha_exp = d.has_alpha ? (int32_t)f.ec[f.alpha_index].exp_bits : 0;
    d.out_bits = 8 * (int32_t)OutBytesPerSample(f); d.out_float = f.exp_bits ? 1 : 0;
    d.unpremultiply = (d.has_alpha && f.ec[f.alpha_index].alpha_associated) ? 1 : 0;
    d.alpha_unit = d.alpha_exp ? 1.0f : 1.0f / (float)((1u << d.alpha_bits) - 1);
    d.dec_gy0 = fp.dec_gy0; d.dec_gy1 = fp.dec_gy1; d.band_y0 = fp.band_y0; d.band_y1 = fp.band_y1;
    const ColorPlan color = PlanColor(f);
    d.to_srgb = color.transfer;   // 0 linear, 1 sRGB, 2 BT.709, 3 PQ, 5 tables
    d.pq_scale = f.intensity_target * 1e-4f;
    d.sec_off = blob.Put(f.sec_off.data(), f.sec_off.size());
    d.sec_size = blob.Put(f.sec_size.data(), f.sec_size.size());
    d.hf_order = put_order(i, f.ng);
    d.tree = blob.Put(f.tree.data(), f.tree.size());
    d.tree_size = (int32_t)f.tree.size();
    PackCode(f.mcode, blob, d.mcode);
    if (plan.global_direct && !f.mcode.use_prefix && !f.mcode.lz77 && f.mcode.num_hist <= 8)
      d.mcode.direct = blob.Fill<uint32_t>((size_t)f.mcode.num_hist << 12, [&](uint32_t* h) { BuildDirectTable(f.mcode, h); });
    if (in.dev_data && in.dev_data[i] && f.cs_contiguous) d.cs = in.dev_data[i] + f.cs_file_offset;   // the file is resident
    else if (!f.is_layer) d.cs = blob.Put(f.cs, f.cs_size, f.cs_size + 16);
    else {
      const int file = (*in.file_of)[i];
      if (!file_cs_put[file]) { file_cs[file] = blob.Put(f.cs, f.cs_size, f.cs_size + 16); file_cs_put[file] = 1; }
      d.cs = file_cs[file];
    }
    d.cs_size = f.cs_size;
    d.status = ElementAt(out.status_base, (size_t)i * 16);
    out.status_off[i] = wz.OffsetOf(d.status);
    // Where the frame's output kernel writes: the caller's buffer, or scratch.  A frame of a layered image goes to the compositor (f32
    // samples, or output-type samples when every frame replaces: a VarDCT frame is never f32, checked on the host).  A Modular frame
    // decoded at reduced size leaves its full-size samples for box_reduce_kernel (lf_output_kernel needs none).  The reference's decoder
    // library hands out the image as displayed (orientation applied; it is only kept when the caller asks, which
    // Decoder/DecoderContext.cpp never does): such frames are re-laid out at the end (reduced size: stored at the oriented position).
    // (A frame of a layered file is decoded with orientation 1 - the compositor orients - so it needs one scratch image, never two.)
    const bool to_scratch = f.is_layer || (ds ? f.encoding == 1 : f.orientation != 1);
    d.out = to_scratch ? ws.Array<uint8_t>(pixels * OutSamplesPerPixel(f) * (f.layer_f32 ? 4 : OutBytesPerSample(f))) : in.dev_out[i];
    if (ds) d.ds_out = in.dev_out[i];
    if (f.encoding == 1) {
      // Modular (lossless) frame: whole-image int32 channel planes, no VarDCT workspace
      d.is_modular = 1;
      d.w8 = d.h8 = d.wt = d.ht = d.wp = d.hp = 0;   // nothing of the VarDCT pipeline runs for this image
      d.cmyk = f.black_index >= 0 ? 1 : 0;
      d.black_bits = d.cmyk ? (int32_t)f.ec[f.black_index].bits : 8;
      d.nch_out = d.ncolor + d.cmyk + d.has_alpha;
      d.mod_nch = d.nch_out;
      // stream order: colour channels, then the extra channels as listed; output order: colour, black, alpha
      for (int c = 0; c < d.ncolor; c++) d.mod_out_pos[c] = c;
      if (d.cmyk) d.mod_out_pos[d.ncolor + f.black_index] = d.ncolor;
      if (d.has_alpha) d.mod_out_pos[d.ncolor + f.alpha_index] = d.nch_out - 1;
      d.group_dim = (int32_t)f.group_dim;
      d.single = f.single ? 1 : 0;
      d.mod_data_bits = f.mod_data_bits;
      // without Squeeze (at most four colour transforms) the RCTs are undone inside modular_out_kernel; otherwise every inverse
      // operation is its own launch and the output kernel only clamps and interleaves
      const bool inline_rct = !f.mod_has_squeeze && !f.mod_has_palette && f.mod_transforms.size() <= 4;
      d.mod_ntr = inline_rct ? (int32_t)f.mod_transforms.size() : 0;
      for (int t = 0; t < d.mod_ntr; t++) { d.mod_tr[t][0] = (int32_t)f.mod_transforms[t].begin_c; d.mod_tr[t][1] = (int32_t)f.mod_transforms[t].rct_type; }
      std::vector<int32_t*> planes;
      for (auto& pl : f.mod_planes) planes.push_back(ws.Array<int32_t>((size_t)std::max(1, pl.w) * std::max(1, pl.h)));
      for (int c = 0; c < d.mod_nch; c++) d.mod_plane[c] = planes[c];
      const size_t nsec = 1 + (size_t)f.nlf + f.ng;
      d.mod_chan = blob.Fill<ModChanDev>(f.mod_coded.size(), [&](ModChanDev* h) {
        for (auto& ch : f.mod_coded) *h++ = ModChanDev{ch.w, ch.h, ch.hshift, ch.vshift, planes[ch.plane]};
      });
      d.mod_ncoded = (int32_t)f.mod_coded.size();
      d.mod_first_group = (int32_t)f.mod_first_group_channel;
      d.mod_desc = ws.Array<ChanDesc>(nsec * f.mod_coded.size());
      if (f.tree_uses_wp) {
        // weighted-predictor state per section: as wide as the widest channel a section decodes.  A group's rectangle is at most
        // group_dim wide; a palette's meta channel (GlobalModular stream) is as wide as its colour count, which may be more
        int64_t widest = (int64_t)f.group_dim;
        for (auto& ch : f.mod_coded) if (ch.hshift < 0) widest = std::max<int64_t>(widest, ch.w);
        d.wp_grp_ints = 10 * (widest + 2);
        d.wp_grp = ws.Array<int32_t>(nsec * (size_t)d.wp_grp_ints);
      }
      if (f.mcode.lz77) d.lz_mod = ws.Array<uint32_t>(nsec << 20);
      if (!inline_rct)
        for (auto& op : f.mod_ops) {
          const ParsedFrame::ModPlane &pa = f.mod_planes[op.a], &pb = f.mod_planes[op.b];
          ModLaunch ml{op.kind, planes[op.a], planes[op.b], planes[op.c], pa.w, pa.h, pb.w, pb.h, op.type, {nullptr, nullptr, nullptr, nullptr}, op.nout, d.status};
          for (int k = 0; k < op.nout && k < 4; k++) ml.out[k] = planes[op.out[k]];
          out.mod_ops.push_back(ml);
        }
      if (ds) {
        d.ds = 8; d.ds_w = ((int32_t)f.xsize + 7) / 8; d.ds_h = ((int32_t)f.ysize + 7) / 8; d.ds_orient = (int32_t)f.orientation;
        out.max_ds_cells = std::max(out.max_ds_cells, (size_t)d.ds_w * d.ds_h);
      }
      if (f.layer_f32) {   // unclamped f32 samples in the image's colour space; un-premultiply waits for the compositor
        d.out_bits = 32; d.out_float = 1; d.unpremultiply = 0;
      }
      out.max_mod_pixels = std::max(out.max_mod_pixels, pixels);
      continue;
    }
    PackCode(f.acode, blob, d.acode);
    if (f.mcode.lz77) { d.lz_lf = ws.Array<uint32_t>((size_t)f.nlf << 20); d.lz_grp = ws.Array<uint32_t>((size_t)f.ng << 16); }
    if (f.acode.lz77) d.lz_hf = ws.Array<uint32_t>((size_t)f.ng << 18);
    d.num_presets = f.num_presets;
    d.num_block_ctx = f.num_block_ctx;
    memcpy(d.block_ctx_map, f.block_ctx_map.data(), std::min(sizeof(d.block_ctx_map), f.block_ctx_map.size()));
    d.n_qf = (int32_t)f.qf_thr.size();
    d.num_lf_ctx = 1;
    for (int j = 0; j < 3; j++) {
      d.n_lf_thr[j] = (int32_t)std::min<size_t>(15, f.lf_thr[j].size());
      for (int k = 0; k < d.n_lf_thr[j]; k++) d.lf_thr[j][k] = f.lf_thr[j][k];
      d.num_lf_ctx *= d.n_lf_thr[j] + 1;
    }
    for (size_t k = 0; k < f.qf_thr.size() && k < 15; k++) d.qf_thr[k] = f.qf_thr[k];
    for (int o = 0; o < kNumOrders; o++)
      for (int c = 0; c < 3; c++) {
        const std::vector<uint16_t>& own = f.custom_order[o][c];
        d.order[o * 3 + c] = own.empty() ? in.d_natural[o] : blob.Put(own.data(), own.size());
        if (!own.empty()) d.custom_orders = 1;
      }
    d.inv_global_scale = 65536.0f / f.global_scale;
    d.quant_scale = f.global_scale / 65536.0f;
    for (int c = 0; c < 3; c++) d.mul_lf[c] = f.m_lf[c] * (d.inv_global_scale / f.quant_lf);
    d.inv_color_factor = 1.0f / f.color_factor;
    d.lf_cfl_x = f.base_x + f.ytox_lf * d.inv_color_factor;
    d.lf_cfl_b = f.base_b + f.ytob_lf * d.inv_color_factor;
    d.base_x = f.base_x; d.base_b = f.base_b;
    d.x_dm = std::pow(0.8f, (float)f.x_qm_scale - 2.0f);
    d.b_dm = std::pow(0.8f, (float)f.b_qm_scale - 2.0f);
    memcpy(d.qbias, f.qbias, sizeof(d.qbias));
    const std::vector<float>* own_dq[kNumQuantTables];   // the frame's own dequantisation table (null: the library's)
    for (int q = 0; q < kNumQuantTables; q++) {
      own_dq[q] = (!f.dq_default && f.custom_dq[q].size() == 3 * (size_t)in.dq_n[q]) ? &f.custom_dq[q] : nullptr;
      d.dq[q] = own_dq[q] ? blob.Put(own_dq[q]->data(), own_dq[q]->size()) : in.d_dq[q];
      d.dq_n[q] = in.dq_n[q];
      d.scan[q] = scan_list(q, f.custom_order, own_dq[q]);
    }
    if (color.transfer == 5) d.trc_lut = blob.Put(color.trc_lut.data(), (size_t)3 * 4096);
    d.gab = f.gab; d.epf_iters = f.epf_iters; d.skip_lf_smoothing = (f.flags & 128) ? 1 : 0;
    for (int c = 0; c < 3; c++) {
      float div = 1.0f + 4.0f * (f.gab_w1[c] + f.gab_w2[c]);
      d.gab_w[c][0] = 1.0f / div; d.gab_w[c][1] = f.gab_w1[c] / div; d.gab_w[c][2] = f.gab_w2[c] / div;
    }
    memcpy(d.epf_sharp_lut, f.epf_sharp_lut, sizeof(d.epf_sharp_lut));
    memcpy(d.epf_channel_scale, f.epf_channel_scale, sizeof(d.epf_channel_scale));
    d.epf_quant_mul = f.epf_quant_mul; d.epf_pass0_sigma_scale = f.epf_pass0_sigma_scale;
    d.epf_pass2_sigma_scale = f.epf_pass2_sigma_scale; d.epf_border_sad_mul = f.epf_border_sad_mul;
    // linear RGB of the image's own primaries, relative to its intensity target: change of primaries folded into the inverse opsin matrix
    for (int r = 0; r < 3; r++)
      for (int k = 0; k < 3; k++) {
        double a = 0;
        for (int j = 0; j < 3; j++) a += (double)color.from_srgb[r * 3 + j] * (double)f.opsin_inv[j * 3 + k];
        d.opsin_inv[r * 3 + k] = (float)a * (255.0f / f.intensity_target);
      }
    for (int k = 0; k < 3; k++) { d.opsin_bias[k] = f.opsin_bias[k]; d.opsin_bias_cbrt[k] = std::cbrt(f.opsin_bias[k]); }
    // planes
    d.cellinfo = wz.Array<uint32_t>(cells);
    // entry lists of the decoded group rows only (a band decode touches a band's worth), block index for the whole cell grid; a frame
    // whose HF tokens nobody reads (reduced size, no alpha) has neither
    const size_t entries = (size_t)std::max(1, fp.dec_gy1 - fp.dec_gy0) * f.xg * kGroupEntriesCap;
    if (fp.hf) { d.centries = ws.Array<uint32_t>(entries); d.cblk = ws.Array<U32x2>(3 * cells); }
    d.centries_g0 = d.dec_gy0 * (int32_t)f.xg;
    for (int c = 0; c < 3; c++) {
      const ChunkPlanes& p = chunk[(size_t)(i % pixel_chunk) * 3 + c];
      d.lf[c] = ws.Array<float>(cells); d.lf_tmp[c] = ws.Array<float>(cells); d.lfq[c] = ws.Array<int32_t>(cells);
      d.lf_final[c] = d.skip_lf_smoothing ? d.lf[c] : d.lf_tmp[c];
      if (ds) continue;   // no pixel planes: the image is lf_final
      d.coef[c] = p.coef; d.tmp[c] = p.tmp; d.xyb[c] = p.xyb;
      d.xyb2[c] = (float*)d.coef[c];   // the dense coefficient planes (generic path only) are dead once the frame is reconstructed
    }
    if (ds) {
      d.ds = 8; d.ds_w = (int32_t)f.w8; d.ds_h = (int32_t)f.h8; d.ds_orient = (int32_t)f.orientation;
      out.max_ds_cells = std::max(out.max_ds_cells, cells);
    }
    if (f.has_noise && !ds) {   // (a cell is coarser than the noise's 5x5 support: a reduced-size decode adds none)
      // the generator fills the group rows the band's 5x5 support reaches: the band's rows and one more each side, like the decode
      d.has_noise = 1; d.noise_gy0 = d.dec_gy0; d.noise_gy1 = d.dec_gy1;
      d.noise_seed[0] = f.noise_seed[0]; d.noise_seed[1] = f.noise_seed[1];
      memcpy(d.noise_lut, f.noise_lut, sizeof(d.noise_lut));
      for (int c = 0; c < 3; c++) { d.noise_rnd[c] = d.tmp[c]; d.noise[c] = chunk[(size_t)(i % pixel_chunk) * 3 + c].noise; }
      out.any_noise = true;
    }
    d.lf_extra = ws.Array<uint8_t>(f.nlf);
    d.rawq = ws.Array<uint16_t>(cells);
    d.sharp = ws.Array<uint8_t>(cells);
    d.ytox = ws.Array<int8_t>(tiles);
    d.ytob = ws.Array<int8_t>(tiles);
    d.binfo = ws.Array<int32_t>((size_t)f.nlf * kBinfoInts);
    d.lf_desc = ws.Array<ChanDesc>((size_t)f.nlf * 8);
    d.lf_count = ws.Array<uint32_t>(f.nlf);
    d.alpha_desc = ws.Array<ChanDesc>(f.ng);
    d.blk_list = ws.Array<uint32_t>((size_t)f.ng * 1024);
    d.blk_count = ws.Array<uint32_t>(f.ng);
    d.grp_bitpos = ws.Array<uint64_t>(f.ng);
    d.tile_list = ws.Array<uint32_t>(tiles);
    d.alpha32 = ws.Array<int32_t>(pixels);
    d.inv_sigma = ws.Array<float>(cells);
    d.alpha = ws.Array<uint8_t>(pixels * OutBytesPerSample(f));
    if (ds && f.alpha_index >= 0) d.ds_alpha = ws.Array<uint8_t>(cells * OutBytesPerSample(f));
    d.lf_end_bits = ws.Array<uint64_t>(1);
    // a frame of one group has its alpha channel in LfGlobal (channels no larger than a group are coded globally)
    d.alpha_in_global = (d.has_alpha && f.ng == 1) ? 1 : 0;
    d.lf_start_bits = f.after_lf_global_bits;
    if (f.single) {
      d.single = 1;
      d.hf_start_bits = f.hf_start_bits;
    }
    if (f.tree_uses_wp) { d.wp_grp_ints = 10 * (kGroupDim + 2); d.wp_lf = ws.Array<int32_t>((size_t)f.nlf * kWpLfInts); d.wp_grp = ws.Array<int32_t>((size_t)f.ng * d.wp_grp_ints); }
    // Loop-filter routing.  Frames with EPF iterations run iteration 1 (+ Gaborish when no iteration 0 has to come between them) and
    // iteration 2 in the streaming kernels: fused_gab_epf1 = 1: one kernel -> output; 2: two kernels, f32 rows (stream_mid) between
    // them.  Three iterations (distance >= 4): Gaborish and iteration 0 first, as LDS-tiled stage kernels, then the two streaming
    // kernels without Gaborish (stream_no_gab).  Stage kernels ping-pong between xyb and xyb2 (the dead dense-coefficient planes).
    float** cur = d.xyb;
    float** other = d.xyb2;
    d.fused_gab_epf1 = (!in.debug_taps && f.epf_iters >= 1) ? (f.epf_iters == 1 ? 1 : 2) : 0;
    d.stream_no_gab = (d.fused_gab_epf1 && (!f.gab || f.epf_iters == 3)) ? 1 : 0;
    d.stage_on[0] = (f.gab && (!d.fused_gab_epf1 || f.epf_iters == 3)) ? 1 : 0;
    d.stage_on[1] = f.epf_iters == 3;
    d.stage_on[2] = f.epf_iters >= 1 && !d.fused_gab_epf1;
    d.stage_on[3] = f.epf_iters >= 2 && !d.fused_gab_epf1;
    d.stage_on[4] = 1;
    for (int s = 0; s < 5; s++) {
      if (s == 2) for (int c = 0; c < 3; c++) { d.stream_in[c] = cur[c]; d.stream_mid[c] = other[c]; }
      for (int c = 0; c < 3; c++) { d.stage_in[s][c] = cur[c]; d.stage_out[s][c] = other[c]; }
      if (s < 4 && d.stage_on[s]) std::swap(cur, other);
    }
    d.final_stage = 4;
    for (int s = 0; s < 4; s++) if (d.stage_on[s]) d.final_stage = s;
    if (in.debug_taps) d.final_stage = 4;   // keep the filtered float planes for the stage taps; out_only_kernel converts
    // the layouts the two-pixels-per-lane kernels handle: even width; 8-bit RGBA / RGB / gray + alpha / gray output (bit 0: the Gaborish + first
    // iteration kernel, which for a two-iteration frame writes f32 rows whatever the output; bit 1: the second iteration's kernel)
    {
      // (their buffer resources address 2 GB from a plane's base: larger planes take the general kernels)
      const bool even = d.fused_gab_epf1 && (d.w & 1) == 0 && d.w >= 8 && !in.no_stream_pairs && (uint64_t)d.wp * (uint64_t)d.hp * 4u < (1ull << 31);
      // 8-bit samples, sRGB or linear: RGBA, RGB, gray + alpha, gray (a frame's channel count is ncolor + has_alpha)
      const bool rgba8 = d.out_bits == 8 && d.to_srgb <= 1 && !d.unpremultiply && (d.ncolor == 3 || d.ncolor == 1) &&
                         d.nch_out == d.ncolor + (d.has_alpha ? 1 : 0) && !d.cmyk;
      d.stream_pairs = (even && (d.fused_gab_epf1 == 2 || rgba8) ? 1 : 0) | (even && d.fused_gab_epf1 == 2 && rgba8 ? 2 : 0);
      if (d.has_noise) {
        // noise is added by the general output path: the kernel that writes the pixels is never a pair kernel.  Which conversion to
        // 8 bits the same frame WITHOUT noise would get is kept, so that noise of strength zero changes no byte.
        const int out_bit = d.fused_gab_epf1 == 2 ? 2 : 1;
        d.noise_pairs_twin = (d.stream_pairs & out_bit) ? 1 : 0;
        d.stream_pairs &= ~out_bit;
      }
    }
    if (d.fused_gab_epf1) {
      d.final_stage = 5;
      out.any_fused |= (d.stream_pairs & 1) ? 1 : 2;
      if (d.fused_gab_epf1 == 2) out.any_fused2 |= (d.stream_pairs & 2) ? 1 : 2;
    }
    out.any_unfiltered |= d.final_stage == 4;
    out.max_w = std::max<int>(out.max_w, f.xsize); out.max_h = std::max<int>(out.max_h, f.ysize);
    out.max_tiles = std::max<int>(out.max_tiles, (int)tiles);
    for (int st = 0; st < 4; st++) if (d.stage_on[st]) out.stage_mask |= 1 << st;
    out.any_alpha |= d.has_alpha != 0;
    out.any_vardct = true;
    out.max_cells = std::max(out.max_cells, cells);
    out.max_groups = std::max<int>(out.max_groups, (int)f.ng);
    // progressive frames: one record per further pass, chained from this one.  A pass owns its code, scan lists, entry lists, block
    // index, end positions and LZ77 window; the alpha stream follows the HF tokens of the last pass.
    d.num_passes = (int32_t)f.num_passes;
    d.pass_shift = (int32_t)f.pass_shift[0];
    d.hf_sec_base = 2 + (int32_t)f.nlf;
    d.alpha_sec_base = 2 + (int32_t)f.nlf + (int32_t)((f.num_passes - 1) * f.ng);   // the Modular streams of all shifts below 3 are in the last pass
    d.alpha_bitpos = d.grp_bitpos;
    for (size_t p = 0; p < f.extra_passes.size(); p++) {
      const ParsedFrame::PassCodes& ep = f.extra_passes[p];
      const size_t rec = (size_t)fp.first_extra + p;
      DevImage& sh = imgs[rec];
      sh = d;
      PackCode(ep.acode, blob, sh.acode);
      sh.lz_hf = ep.acode.lz77 ? ws.Array<uint32_t>((size_t)f.ng << 18) : nullptr;
      for (int q = 0; q < kNumQuantTables; q++) sh.scan[q] = scan_list(q, ep.custom_order, own_dq[q]);
      if (fp.hf) { sh.centries = ws.Array<uint32_t>(entries); sh.cblk = ws.Array<U32x2>(3 * cells); }
      sh.grp_bitpos = ws.Array<uint64_t>(f.ng);
      sh.hf_order = put_order(rec, f.ng);
      sh.pass_shift = p + 1 < f.num_passes - 1 ? (int32_t)f.pass_shift[p + 1] : 0;
      sh.hf_sec_base = 2 + (int32_t)f.nlf + (int32_t)((p + 1) * f.ng);
      sh.next_pass = nullptr;
      (p ? imgs[rec - 1] : d).next_pass = ElementAt(out.d_imgs, rec);
    }
    if (!f.extra_passes.empty()) {
      d.alpha_bitpos = imgs[(size_t)fp.first_extra + f.extra_passes.size() - 1].grp_bitpos;
      for (size_t p = 0; p < f.extra_passes.size(); p++) imgs[(size_t)fp.first_extra + p].alpha_bitpos = d.alpha_bitpos;
    }
  }
  // the plan's task tables
  auto put_tasks = [&](const std::vector<SectionTask>& t) { return blob.Put(t.data(), t.size(), 1); };
  out.lf_tasks = put_tasks(plan.lf_finish_tasks);
  out.pass_tasks = put_tasks(plan.pass_tasks);
  out.lf_ans_tasks = put_tasks(plan.lf_ans_tasks);
  out.mod_tasks = put_tasks(plan.mod_tasks);
  out.alpha_tasks = put_tasks(plan.alpha_tasks);
  if (in.comps && !in.comps->empty()) {
    // the compositor's tables: one record per layered image, one per frame (frame records indexed like the batch's images)
    const std::vector<Composite>& comps = *in.comps;
    for (size_t k = 0; k < comps.size(); k++)   // compose_kernel: 256-pixel row segments
      out.max_segments = std::max(out.max_segments, (int)(*in.files)[k].ysize * (int)(((*in.files)[k].xsize + 255) / 256));
    for (size_t k = 0; k < comps.size(); k++) {   // compose_reduce_kernel: 8x8 cells of the displayed image (transposing swaps its sides)
      const ParsedFrame& top = (*in.files)[k];
      if (!top.layers->reduce) continue;
      out.compose_reduce = true;
      out.max_reduce_cells = std::max(out.max_reduce_cells, (int)((top.xsize + 7) / 8) * (int)((top.ysize + 7) / 8));
    }
    out.comp_imgs = blob.Fill<ComposeImage>(comps.size(), [&](ComposeImage* cimgs) {
      for (size_t k = 0; k < comps.size(); k++) {
        const ParsedFrame& top = (*in.files)[k];
        ComposeImage& ci = cimgs[k];
        memset(&ci, 0, sizeof(ci));
        ci.w = (int32_t)top.xsize; ci.h = (int32_t)top.ysize;
        ci.has_alpha = top.alpha_index >= 0 ? 1 : 0;
        ci.nch = top.ncolor + ci.has_alpha;
        ci.premul = (ci.has_alpha && top.ec[top.alpha_index].alpha_associated) ? 1 : 0;
        ci.orientation = (int32_t)top.orientation;
        ci.out_bits = 8 * (int32_t)OutBytesPerSample(top); ci.out_float = top.exp_bits ? 1 : 0;
        ci.first = comps[k].first; ci.count = comps[k].count;
        ci.raw = top.layers->raw ? 1 : 0;
        ci.out = comps[k].out;
        ci.live_in = top.layers->live_in; ci.live_out = top.layers->live_out;
        ci.slots_in = top.layers->slots_in; ci.slots_out = top.layers->slots_out;
        for (int s = 0; s < 4; s++) ci.slot_plane[s] = top.layers->slot_plane[s];
        ci.out_stride = top.layers->out_stride;
        ci.reduce = top.layers->reduce ? 1 : 0;
      }
    });
    out.comp_frames = blob.Fill<ComposeFrame>((size_t)n, [&](ComposeFrame* cframes) {
      for (size_t k = 0; k < comps.size(); k++) {
        const Composite& c = comps[k];
        const ParsedFrame& top = (*in.files)[k];
        for (int j = 0; j < c.count; j++) {
          const ParsedFrame& f = frames[c.first + j];
          ComposeFrame& cf = cframes[c.first + j];
          memset(&cf, 0, sizeof(cf));
          cf.px = (const float*)imgs[c.first + j].out;
          cf.x0 = f.have_crop ? f.crop_x0 : 0; cf.y0 = f.have_crop ? f.crop_y0 : 0;
          cf.w = (int32_t)f.xsize; cf.h = (int32_t)f.ysize;
          const BlendInfo& bc = f.blend[0];
          const BlendInfo& ba = top.alpha_index >= 0 ? f.blend[1 + top.alpha_index] : bc;
          cf.mode[0] = (int32_t)bc.mode; cf.mode[1] = (int32_t)ba.mode;
          cf.source[0] = (int32_t)bc.source; cf.source[1] = (int32_t)ba.source;
          cf.clamp[0] = (int32_t)bc.clamp; cf.clamp[1] = (int32_t)ba.clamp;
          cf.save = c.save[j];
          cf.show = top.layers->show.empty() ? (j == c.count - 1 ? 0 : -1) : top.layers->show[j];
          // a reference-only frame is read by patches only: an empty crop and no save leave the canvas and the slots as they are
          if (f.frame_type == 2) { cf.w = cf.h = 0; cf.save = -1; cf.show = -1; }
          // a frame that was refused after the file was expanded (its LF pre-pass failed) has no samples: an empty crop, so that the
          // launch reads nothing of it (the file fails through the frame's status)
          if (!decoded(c.first + j)) { cf.px = nullptr; cf.w = cf.h = 0; }
        }
      }
    });
  }
  if (in.patches && !in.patches->tiles.empty()) {
    const PatchTables& T = *in.patches;
    out.patch_frames = blob.Fill<PatchFrame>(T.image.size(), [&](PatchFrame* pfr) {
      for (size_t k = 0; k < T.image.size(); k++) {
        const ParsedFrame& f = frames[T.image[k]];
        PatchFrame& p = pfr[k];
        memset(&p, 0, sizeof(p));
        p.px = (float*)imgs[T.image[k]].out;   // the frame's f32 layer scratch (layer_f32: every frame of an image with patches)
        p.w = (int32_t)f.xsize; p.h = (int32_t)f.ysize;
        p.has_alpha = f.alpha_index >= 0 ? 1 : 0;
        p.nch = f.ncolor + p.has_alpha;
        p.premul = (p.has_alpha && f.ec[f.alpha_index].alpha_associated) ? 1 : 0;
      }
    });
    out.patch_refs = blob.Fill<PatchRef>(T.refs.size(), [&](PatchRef* refs) {
      memcpy(refs, T.refs.data(), sizeof(PatchRef) * T.refs.size());
      for (size_t k = 0; k < T.image.size(); k++)
        for (auto& rr : frames[T.image[k]].patch_refs) {   // in the order BuildPatchTables listed them
          const int atlas = T.first[k] + rr.frame;
          const ParsedFrame& a = frames[atlas];
          refs->px = (const float*)imgs[atlas].out + ((size_t)rr.y0 * a.xsize + rr.x0) * OutSamplesPerPixel(a);
          refs->stride = (int32_t)a.xsize;
          refs++;
        }
    });
    out.patch_pos = blob.Put(T.pos.data(), T.pos.size());
    out.patch_tiles = blob.Put(T.tiles.data(), T.tiles.size());
    out.patch_list = blob.Put(T.list.data(), T.list.size());
  }
  if (DevImage* h = blob.Host(out.d_imgs)) memcpy(h, imgs.data(), sizeof(DevImage) * imgs.size());
}

}  // namespace jxlhip
