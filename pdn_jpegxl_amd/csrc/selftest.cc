// Host-only self tests of the writers (CPU tests, no GPU): the encoder's code builder, MA-tree writer and header writers against the
// decoder's parsers.  TEST INFRASTRUCTURE: compiled into lib/libjxlhip_selftest.so only (build.py), never into the library the
// reference's host loads - the production library exports GetLibJxlVersion / LoadImage / SaveImage and the jxlhip_* batch API, no hooks.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/jxlfiletypeio.h"
#include "animation.h"
#include "dev_util.h"
#include "enc_animation.h"
#include "enc_types.h"
#include "batch_layout.h"
#include "enc_batch_layout.h"
#include "entropy_plan.h"
#include "host_parse.h"
#include "host_write.h"
#include "icc.h"
#include "modular_rules.h"
#include "varblock_rules.h"

namespace jxlhip {
std::vector<EncTreeNode> MakeEncoderTree(uint32_t nlf);
// encoder.cc: the tree and the GlobalModular header of a searched lossless frame (efforts 8 and 9)
extern const int32_t kWpCutsHost[kWpLeaves - 1];
std::vector<EncTreeNode> MakeLosslessSearchTree(int nch, const int32_t* pred, bool wp_ctx, int palette, uint8_t ctx[4][kWpLeaves + 1], int* palette_ctx);
void WriteLosslessSearchHeader(BitWriter& bw, int palette_colours, int palette_channels, int rct_type);
}
using namespace jxlhip;

static void SetEncErr(ErrorInfo* e, const char* msg) {
  if (!e || !msg) return;
  size_t n = strlen(msg);
  if (n == 0) return;
  if (n > 255) n = 255;
  memcpy(e->errorMessage, msg, n);
  e->errorMessage[n] = 0;
}

namespace jxlhip {
bool ReadBackTokens(const uint8_t* bytes, size_t nbytes, size_t num_ctx, const uint32_t* ctxs, const uint32_t* values, size_t n, std::string* why);
bool ReadBackTree(const uint8_t* bytes, size_t nbytes, std::vector<DevTreeNode>* tree, std::string* why);
}

// Writes n pseudo-random tokens over num_ctx contexts with the encoder's code builder and reads them back with the decoder's
// header parser and symbol reader.  Returns 0 on success (message in err otherwise).
extern "C" JXLFILETYPEIO_API int32_t jxlhip_selftest_entropy(uint32_t seed, uint32_t num_ctx, uint32_t n, int32_t max_clusters,
                                                             uint32_t pinned_ctx_plus1, ErrorInfo* err) {
  try {
    uint64_t s = seed * 0x9E3779B97F4A7C15ull + 12345;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 32); };
    std::vector<uint32_t> ctxs(n), vals(n), hist((size_t)num_ctx * kEncAlphabet, 0);
    std::vector<uint8_t> pinned(num_ctx, 0);
    if (pinned_ctx_plus1) pinned[pinned_ctx_plus1 - 1] = 1;
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t c = rnd() % num_ctx;
      // geometric-ish magnitudes whose spread depends on the context; a few large outliers exercise the extra bits
      uint32_t v = 0;
      const uint32_t spread = 1 + c % 7;
      while ((rnd() % (spread + 1)) != 0 && v < 40) v++;
      if (rnd() % 97 == 0) v = rnd() >> (rnd() % 30);
      if (pinned[c]) v = 0;
      ctxs[i] = c; vals[i] = v;
      uint32_t tok, nb, bits;
      HybridEncode(v, &tok, &nb, &bits);
      hist[(size_t)c * kEncAlphabet + tok]++;
    }
    BitWriter bw;
    EncCode code;
    BuildAndWriteCode(hist.data(), num_ctx, max_clusters, pinned, bw, code);
    std::vector<EncToken> toks;
    for (uint32_t i = 0; i < n; i++)
      if (!pinned[ctxs[i]]) toks.push_back(EncToken{ctxs[i], vals[i]});   // tokens of pinned contexts are never written
    WriteTokensHost(toks, code, bw);
    std::vector<uint8_t> bytes = bw.Finish();
    std::string why;
    // the decoder reads every token, the pinned ones included (they cost no bits and leave the state alone)
    if (!ReadBackTokens(bytes.data(), bytes.size(), num_ctx, ctxs.data(), vals.data(), n, &why)) { SetEncErr(err, why.c_str()); return 1; }
    return 0;
  } catch (const std::exception& e) {
    SetEncErr(err, e.what());
    return 2;
  }
}

// Serialises the encoder's MA tree and parses it back; returns 0 when node for node identical.
extern "C" JXLFILETYPEIO_API int32_t jxlhip_selftest_tree(uint32_t nlf, ErrorInfo* err) {
  try {
    const std::vector<EncTreeNode> t = MakeEncoderTree(nlf);
    BitWriter bw;
    WriteTree(t, bw);
    std::vector<uint8_t> bytes = bw.Finish();
    std::vector<DevTreeNode> back;
    std::string why;
    if (!ReadBackTree(bytes.data(), bytes.size(), &back, &why)) { SetEncErr(err, why.c_str()); return 1; }
    if (back.size() != t.size()) { SetEncErr(err, "node count"); return 2; }
    uint32_t leaf = 0;
    for (size_t i = 0; i < t.size(); i++) {
      if (t[i].property >= 0) {
        if (back[i].property != t[i].property || back[i].splitval != t[i].splitval) { SetEncErr(err, "inner node"); return 3; }
      } else {
        if (back[i].property >= 0 || (back[i].a & 0xFF) != (uint32_t)t[i].pred || (back[i].a >> 8) != leaf || back[i].splitval != t[i].offset ||
            back[i].b != t[i].multiplier) { SetEncErr(err, "leaf"); return 4; }
        leaf++;
      }
    }
    return leaf == kNumEncLeaves ? 0 : 5;
  } catch (const std::exception& e) {
    SetEncErr(err, e.what());
    return 6;
  }
}

// Writes the codestream headers + frame header + TOC the encoder would emit for the given geometry (sections of `sec_bytes` bytes each)
// into dst; the CPU tests read them back with jxlhip_peek (ParseFile, headers only).  Returns the byte count (0 on failure).
extern "C" JXLFILETYPEIO_API size_t jxlhip_selftest_headers(uint32_t xsize, uint32_t ysize, int32_t gray, int32_t alpha, int32_t lossless,
                                                            uint32_t epf_iters, uint32_t sec_bytes, uint8_t* dst, size_t capacity) {
  try {
    EncImageInfo ii;
    ii.xsize = xsize; ii.ysize = ysize; ii.gray = gray != 0; ii.alpha = alpha != 0; ii.xyb = !lossless;
    EncFrameInfo fi;
    fi.encoding = lossless ? 1 : 0;
    fi.gab = !lossless; fi.epf_iters = lossless ? 0 : epf_iters;
    BitWriter cs;
    WriteCodestreamHeaders(ii, cs);
    WriteFrameHeader(ii, fi, cs);
    const uint32_t ng = ((xsize + 255) / 256) * ((ysize + 255) / 256), nlf = ((xsize + 2047) / 2048) * ((ysize + 2047) / 2048);
    std::vector<uint32_t> sizes(ng == 1 ? 1 : 2 + nlf + ng, sec_bytes);
    WriteToc(sizes, cs);
    std::vector<uint8_t> bytes = cs.Finish();
    bytes.resize(bytes.size() + (size_t)sec_bytes * sizes.size(), 0);
    std::vector<uint8_t> file = WriteContainer(bytes, nullptr, 0, nullptr, 0);
    if (file.size() > capacity) return 0;
    memcpy(dst, file.data(), file.size());
    return file.size();
  } catch (...) {
    return 0;
  }
}

// The same for the sample depth and colour encoding of a jxlhip_save_pixels call: bits / exp_bits as the headers state them (8..16 / 0
// integers, 16 / 5 binary16, 32 / 8 binary32), `colour` a KnownColorProfile (the gray ones with gray != 0).
extern "C" JXLFILETYPEIO_API size_t jxlhip_selftest_headers_deep(uint32_t xsize, uint32_t ysize, int32_t gray, int32_t alpha, int32_t lossless,
                                                                 uint32_t bits, uint32_t exp_bits, int32_t colour, uint8_t* dst, size_t capacity) {
  try {
    EncImageInfo ii;
    ii.xsize = xsize; ii.ysize = ysize; ii.gray = gray != 0; ii.alpha = alpha != 0; ii.xyb = !lossless;
    ii.bits = bits; ii.exp_bits = exp_bits;
    switch (colour) {
      case KnownColorProfile_Srgb: case KnownColorProfile_GraySrgbTRC: break;
      case KnownColorProfile_LinearSrgb: case KnownColorProfile_LinearGray: ii.transfer = 8; break;
      case KnownColorProfile_DisplayP3: ii.primaries = 11; break;
      case KnownColorProfile_Rec709: ii.transfer = 1; break;
      case KnownColorProfile_Rec2020Linear: ii.primaries = 9; ii.transfer = 8; break;
      case KnownColorProfile_Rec2020PQ: ii.primaries = 9; ii.transfer = 16; ii.pq_intensity = true; break;
      default: return 0;
    }
    EncFrameInfo fi;
    fi.encoding = lossless ? 1 : 0;
    fi.gab = !lossless; fi.epf_iters = lossless ? 0 : 1;
    BitWriter cs;
    WriteCodestreamHeaders(ii, cs);
    WriteFrameHeader(ii, fi, cs);
    const uint32_t ng = ((xsize + 255) / 256) * ((ysize + 255) / 256), nlf = ((xsize + 2047) / 2048) * ((ysize + 2047) / 2048);
    std::vector<uint32_t> sizes(ng == 1 ? 1 : 2 + nlf + ng, 3);
    WriteToc(sizes, cs);
    std::vector<uint8_t> bytes = cs.Finish();
    bytes.resize(bytes.size() + 3 * sizes.size(), 0);
    std::vector<uint8_t> file = WriteContainer(bytes, nullptr, 0, nullptr, 0);
    if (file.size() > capacity) return 0;
    memcpy(dst, file.data(), file.size());
    return file.size();
  } catch (...) {
    return 0;
  }
}

// The same with an embedded ICC profile (host only: the ICC stream writer against the parser's reader).
extern "C" JXLFILETYPEIO_API size_t jxlhip_selftest_headers_icc(uint32_t xsize, uint32_t ysize, int32_t alpha, int32_t lossless, const uint8_t* icc,
                                                                size_t icc_size, uint8_t* dst, size_t capacity) {
  try {
    EncImageInfo ii;
    ii.xsize = xsize; ii.ysize = ysize; ii.gray = false; ii.alpha = alpha != 0; ii.xyb = !lossless;
    ii.icc = icc; ii.icc_size = icc_size;
    EncFrameInfo fi;
    fi.encoding = lossless ? 1 : 0;
    fi.gab = !lossless; fi.epf_iters = lossless ? 0 : 1;
    BitWriter cs;
    WriteCodestreamHeaders(ii, cs);
    WriteFrameHeader(ii, fi, cs);
    const uint32_t ng = ((xsize + 255) / 256) * ((ysize + 255) / 256), nlf = ((xsize + 2047) / 2048) * ((ysize + 2047) / 2048);
    std::vector<uint32_t> sizes(ng == 1 ? 1 : 2 + nlf + ng, 3);
    WriteToc(sizes, cs);
    std::vector<uint8_t> bytes = cs.Finish();
    bytes.resize(bytes.size() + 3 * sizes.size(), 0);
    std::vector<uint8_t> file = WriteContainer(bytes, nullptr, 0, nullptr, 0);
    if (file.size() > capacity) return 0;
    memcpy(dst, file.data(), file.size());
    return file.size();
  } catch (...) {
    return 0;
  }
}

// The edge rule of the loop filters and the encoder's analysis (dev_util.h ReflectIndex), compiled for the host: index v of a
// dimension of n samples.
extern "C" JXLFILETYPEIO_API int32_t jxlhip_selftest_reflect(int32_t v, int32_t n) { return ReflectIndex(v, n); }

extern "C" JXLFILETYPEIO_API uint32_t jxlhip_selftest_nnz_ctx(uint32_t nzl) { return NnzBucketCtx(nzl); }
extern "C" JXLFILETYPEIO_API uint32_t jxlhip_selftest_hf_pos_ctx(uint32_t ks) { return HfPosCtx(ks); }
extern "C" JXLFILETYPEIO_API uint32_t jxlhip_selftest_hf_nnz_predict(uint32_t bx, uint32_t by, uint32_t above, uint32_t left) {
  return HfNnzPredict(bx, by, above, left);
}
extern "C" JXLFILETYPEIO_API uint32_t jxlhip_selftest_hf_nnz_bucket(uint32_t predicted) { return HfNnzCountBucket(predicted); }
// whether the coefficient of token value u (signed values packed as UnpackSigned unpacks them) fits an entry
extern "C" JXLFILETYPEIO_API int32_t jxlhip_selftest_hf_entry_fits(uint32_t u) { return HfEntryFits(UnpackSigned(u)) ? 1 : 0; }

// An entropy-coded stream of n (context, value) tokens over num_ctx contexts, as the encoder writes its host-side streams (code header
// by BuildAndWriteCode, tokens by WriteTokensHost): the CPU and GPU tests write patch dictionaries with it.  Writes the bytes into dst
// (zero-padded to a byte) and the exact bit count into *nbits; returns the byte count (0 on failure or when dst is too small).
extern "C" JXLFILETYPEIO_API size_t jxlhip_selftest_write_tokens(uint32_t num_ctx, const uint32_t* ctxs, const uint32_t* values, uint32_t n,
                                                                 uint8_t* dst, size_t capacity, uint64_t* nbits) {
  try {
    std::vector<uint32_t> hist((size_t)num_ctx * kEncAlphabet, 0);
    std::vector<EncToken> toks;
    for (uint32_t i = 0; i < n; i++) {
      if (ctxs[i] >= num_ctx) return 0;
      uint32_t tok, nb, bits;
      HybridEncode(values[i], &tok, &nb, &bits);
      hist[(size_t)ctxs[i] * kEncAlphabet + tok]++;
      toks.push_back(EncToken{ctxs[i], values[i]});
    }
    BitWriter bw;
    EncCode code;
    BuildAndWriteCode(hist.data(), num_ctx, (int)num_ctx, std::vector<uint8_t>(num_ctx, 0), bw, code);
    WriteTokensHost(toks, code, bw);
    const uint64_t bit_count = bw.BitCount();
    std::vector<uint8_t> bytes = bw.Finish();
    if (bytes.size() > capacity) return 0;
    memcpy(dst, bytes.data(), bytes.size());
    *nbits = bit_count;
    return bytes.size();
  } catch (...) {
    return 0;
  }
}

// The searched lossless tree (efforts 8 and 9; palette: 0 none, 1 one-group frame, 2 several groups) serialised and parsed back:
// node for node identical, and a walk for every (stream, channel, property-15 value around each threshold) ends in the leaf whose
// context and predictor the encoder's table names.  Returns 0 on success.
extern "C" JXLFILETYPEIO_API int32_t jxlhip_selftest_lossless_tree(int32_t nch, const int32_t* pred, int32_t wp_ctx, int32_t palette, ErrorInfo* err) {
  try {
    uint8_t ctx[4][kWpLeaves + 1];
    int pal_ctx = -1;
    const std::vector<EncTreeNode> t = MakeLosslessSearchTree(nch, pred, wp_ctx != 0, palette, ctx, &pal_ctx);
    BitWriter bw;
    WriteTree(t, bw);
    std::vector<uint8_t> bytes = bw.Finish();
    std::vector<DevTreeNode> back;
    std::string why;
    if (!ReadBackTree(bytes.data(), bytes.size(), &back, &why)) { SetEncErr(err, why.c_str()); return 1; }
    if (back.size() != t.size()) { SetEncErr(err, "node count"); return 2; }
    for (size_t i = 0; i < t.size(); i++) {
      if (t[i].property >= 0 ? (back[i].property != t[i].property || back[i].splitval != t[i].splitval)
                             : (back[i].property >= 0 || (back[i].a & 0xFF) != (uint32_t)t[i].pred || back[i].b != 1 || back[i].splitval != 0)) {
        SetEncErr(err, "node differs");
        return 3;
      }
    }
    auto walk = [&](int stream, int chan, int64_t p15) {
      size_t node = 0;
      while (back[node].property >= 0) {
        const int64_t v = back[node].property == 0 ? chan : (back[node].property == 1 ? stream : p15);
        if (back[node].property != 0 && back[node].property != 1 && back[node].property != 15) throw std::runtime_error("unexpected property");
        node = v > back[node].splitval ? back[node].a : back[node].b;
      }
      return back[node].a;   // context << 8 | predictor
    };
    for (int c = 0; c < nch; c++)
      for (int k = 0; k < kWpLeaves; k++) {
        // the values of bucket k: above threshold k - 1, up to threshold k
        const int64_t lo = k ? (int64_t)kWpCutsHost[k - 1] + 1 : -100000, hi = k < kWpLeaves - 1 ? (int64_t)kWpCutsHost[k] : 100000;
        for (int64_t v : {lo, hi}) {
          const int chan = palette == 1 ? c + 1 : c, stream = palette == 2 ? 21 : 0;
          const uint32_t leaf = walk(stream, chan, v);
          if ((leaf >> 8) != ctx[c][wp_ctx ? k : 0] || (leaf & 0xFF) != (uint32_t)pred[c]) { SetEncErr(err, "a walk ends in another leaf than the table says"); return 4; }
        }
      }
    if (palette) {
      const uint32_t leaf = walk(0, 0, 0);
      if ((int)(leaf >> 8) != pal_ctx || (leaf & 0xFF) != (uint32_t)pred[nch]) { SetEncErr(err, "the palette's leaf"); return 5; }
    }
    return 0;
  } catch (const std::exception& e) {
    SetEncErr(err, e.what());
    return 6;
  }
}

// A whole one-group lossless file (bare codestream) written by the host pieces of efforts 8 and 9, for the CPU tests to parse and to
// decode with the oracle.  palette_colours > 0: nch channels through a palette whose colour i has (37 i + 91 c) & 255 in channel c, the
// pixel (x, y) showing colour (x + 2 y) % palette_colours, indices under the gradient predictor.  palette_colours == 0: every sample
// zero, under the effort-9 tree (weighted predictor, property-15 contexts; on zeros both are 0, which needs no predictor state here).
// Returns the byte count (0 on failure).
extern "C" JXLFILETYPEIO_API size_t jxlhip_selftest_lossless_file(uint32_t w, uint32_t h, int32_t nch, int32_t palette_colours, uint8_t* dst,
                                                                  size_t capacity) {
  try {
    if (!w || !h || w > 256 || h > 256 || nch < 1 || nch > 4 || palette_colours < 0 || palette_colours > 256) return 0;
    uint8_t ctx[4][kWpLeaves + 1];
    int pal_ctx = -1;
    std::vector<EncToken> toks;
    std::vector<EncTreeNode> tree;
    if (palette_colours) {
      const int32_t pred[2] = {5, 1};
      tree = MakeLosslessSearchTree(1, pred, false, 1, ctx, &pal_ctx);
      auto pack = [](int32_t v) { return v >= 0 ? (uint32_t)v << 1 : ((uint32_t)(-v) << 1) - 1; };
      for (int c = 0; c < nch; c++)   // the colours: West predictor, the first of a row from the row above
        for (int i = 0; i < palette_colours; i++) {
          const int32_t v = (37 * i + 91 * c) & 255, W = i ? (37 * (i - 1) + 91 * c) & 255 : (c ? (91 * (c - 1)) & 255 : 0);
          toks.push_back(EncToken{(uint32_t)pal_ctx, pack(v - W)});
        }
      auto at = [&](int x, int y) { return (int32_t)((x + 2 * y) % palette_colours); };
      for (int y = 0; y < (int)h; y++)
        for (int x = 0; x < (int)w; x++) {
          const int32_t W = x ? at(x - 1, y) : (y ? at(0, y - 1) : 0), N = x && y ? at(x, y - 1) : W, NW = x && y ? at(x - 1, y - 1) : W;
          const int32_t gr = W + N - NW, guess = std::max(std::min(W, N), std::min(std::max(W, N), gr));
          toks.push_back(EncToken{ctx[0][0], pack(at(x, y) - guess)});
        }
    } else {
      const int32_t pred[4] = {6, 6, 6, 6};
      tree = MakeLosslessSearchTree(nch, pred, true, 0, ctx, nullptr);
      for (int c = 0; c < nch; c++)
        for (uint32_t i = 0; i < w * h; i++) toks.push_back(EncToken{ctx[c][5], 0});   // property 15 = 0 exceeds five thresholds
    }
    const size_t leaves = (tree.size() + 1) / 2;
    std::vector<uint32_t> hist(leaves * kEncAlphabet, 0);
    for (auto& t : toks) { uint32_t tok, nb, bits; HybridEncode(t.value, &tok, &nb, &bits); hist[(size_t)t.ctx * kEncAlphabet + tok]++; }
    BitWriter g;
    EncCode code;
    g.Bool(true);   // default LF dequantisation factors
    g.Bool(true);   // global MA tree
    WriteTree(tree, g);
    BuildAndWriteCode(hist.data(), leaves, 12, {}, g, code);
    WriteLosslessSearchHeader(g, palette_colours, nch, -1);
    WriteTokensHost(toks, code, g);
    EncImageInfo ii;
    ii.xsize = w; ii.ysize = h; ii.gray = nch < 3; ii.alpha = nch == 2 || nch == 4; ii.xyb = false;
    EncFrameInfo fi;
    fi.encoding = 1; fi.group_size_shift = 1; fi.gab = false; fi.epf_iters = 0;
    BitWriter cs;
    WriteCodestreamHeaders(ii, cs);
    WriteFrameHeader(ii, fi, cs);
    std::vector<uint8_t> sec = g.Finish();
    WriteToc({(uint32_t)sec.size()}, cs);
    std::vector<uint8_t> bytes = cs.Finish();
    bytes.insert(bytes.end(), sec.begin(), sec.end());
    if (bytes.size() > capacity) return 0;
    memcpy(dst, bytes.data(), bytes.size());
    return bytes.size();
  } catch (...) {
    return 0;
  }
}

// The LDS layouts of the entropy kernels (lds_layout.h) as numbers, for tests/test_entropy_plan.py.  in: the numbers a layout is made
// from, a code's shape being (clusters, log_alpha, contexts, prefix); out: its pieces' offsets in carving order, its end, then the sizes
// the host launches with.  Returns how many numbers it wrote (0: unknown kind).
//   0 code          in: off, shape                                   out: alias, cfg, cmap, end | CodeLdsBytes
//   1 tree + code   in: off, nodes, shape                            out: tree, alias, cfg, cmap, end | ModTablesLdsBytes
//   2 lf / alpha    in: slots, nodes, shape                          out: windows, tree, alias, cfg, cmap, end | SlotsLdsBytes, lanes only
//   3 Modular       in: lanes, rb_width, wp_lds, uniform, nodes, shape   out: windows, rows, wp, grid, tree, alias, cfg, cmap, end | ModularLdsBytes, lanes only
//   4 HF            in: sections, shape                              out: ring, descq, nzcol, alias, cfg, cmap, nnz, end | tables + lanes, lanes only, slots
//   6 alpha rows    in: slots, nodes, shape                          out: tables' end, rows, end | SlotsLdsBytes + AlphaRowsLdsBytes, behind the windows alone: rows, end
//   5 constants     out: kLdsMax, kRingWords, kHfRingWords, kNzColBytes, kNnzCtxBytes, kWpStateInts, kUniRows, kUniGridBytes, sizeof(DevTreeNode)
extern "C" JXLFILETYPEIO_API int32_t jxlhip_selftest_lds_layout(int32_t kind, const int64_t* in, int64_t* out) {
  int k = 0;
  auto put = [&](size_t v) { out[k++] = (int64_t)v; };
  auto shape = [&](int at) { return CodeShape{(uint32_t)in[at], (uint32_t)in[at + 1], (uint32_t)in[at + 2], in[at + 3] != 0}; };
  auto put_code = [&](const CodeLds& c) { put(c.alias); put(c.cfg); put(c.cmap); };
  if (kind == 0) {
    const CodeLds c((size_t)in[0], shape(1));
    put_code(c); put(c.end); put(CodeLdsBytes(shape(1)));
  } else if (kind == 1) {
    const ModTablesLds t((size_t)in[0], (size_t)in[1], shape(2));
    put(t.tree); put_code(CodeLds(t.code, shape(2))); put(t.end); put(ModTablesLdsBytes((size_t)in[1], shape(2)));
  } else if (kind == 2) {
    const SlotsLds l((int)in[0]);
    const ModTablesLds t(l.tables, (size_t)in[1], shape(2));
    put(0); put(t.tree); put_code(CodeLds(t.code, shape(2))); put(t.end);
    put(SlotsLdsBytes((int)in[0], (size_t)in[1], shape(2))); put(l.tables);
  } else if (kind == 3) {
    const ModularLds l((int)in[0], (int)in[1], (int)in[2], in[3] != 0);
    const ModTablesLds t(l.tables, (size_t)in[4], shape(5));
    put(0); put(l.rows); put(l.wp); put(l.grid); put(t.tree); put_code(CodeLds(t.code, shape(5))); put(t.end);
    put(ModularLdsBytes((int)in[0], (int)in[1], (int)in[2], in[3] != 0, (size_t)in[4], shape(5)));
    put(ModularLds((int)in[0], (int)in[1], (int)in[2], false).tables);
  } else if (kind == 4) {
    const int nslots = HfSlots((int)in[0]);
    const HfLds l(nslots);
    const CodeLds c(l.tables, shape(1));
    put(l.ring); put(l.descq); put(l.nzcol); put_code(c); put(c.end); put(HfTablesEnd(l.tables, shape(1)));
    put(HfTablesBytes(shape(1)) + HfLaneBytes(nslots)); put(HfLaneBytes(nslots)); put((size_t)nslots);
  } else if (kind == 6) {
    const SlotsLds l((int)in[0]);
    const ModTablesLds t(l.tables, (size_t)in[1], shape(2));
    const AlphaRowsLds r(t.end, (int)in[0]), g(l.tables, (int)in[0]);
    put(t.end); put(r.rows); put(r.end); put(SlotsLdsBytes((int)in[0], (size_t)in[1], shape(2)) + AlphaRowsLdsBytes((int)in[0]));
    put(g.rows); put(g.end);
  } else if (kind == 5) {
    put(kLdsMax); put(kRingWords); put(kHfRingWords); put(kNzColBytes); put(kNnzCtxBytes); put(kWpStateInts); put(kUniRows); put(kUniGridBytes);
    put(sizeof(DevTreeNode));
  }
  return k;
}

// Parses n files on the host and plans their batch's entropy stage (entropy_plan.h; nothing touches a GPU).  opts: band first row, band
// rows, downscale, lane_stride_override, no_direct, mod_lanes64.  One-group lossy frames are planned without the LF pre-pass that reads
// their HfGlobal (the plan needs no hf_start_bits): their HF code is empty here.  The plan goes to out as numbers, in the order written below; returns
// how many (0: they do not fit `capacity`).
extern "C" JXLFILETYPEIO_API size_t jxlhip_selftest_entropy_plan(int32_t n, const uint8_t* const* data, const size_t* sizes, const int32_t* opts,
                                                                 int64_t* out, size_t capacity) {
  std::vector<ParsedFrame> frames((size_t)n);
  std::vector<int> status((size_t)n, DecoderStatus_Ok);
  for (int i = 0; i < n; i++) {
    try {
      ParseFile(data[i], sizes[i], false, frames[i]);
    } catch (const std::exception&) {
      status[i] = DecoderStatus_DecodeError;
    }
  }
  EntropyPlanOptions o;
  o.band_first_row = opts[0]; o.band_rows = opts[1]; o.downscale = opts[2]; o.lane_stride_override = opts[3];
  o.no_direct = opts[4] != 0; o.mod_lanes64 = opts[5] != 0;
  const EntropyPlan P = PlanEntropy(frames, status, o);
  std::vector<int64_t> v;
  auto put = [&](int64_t x) { v.push_back(x); };
  auto put_shape = [&](const HostCode& hc) { const CodeShape s = ShapeOf(hc); put(s.clusters); put(s.log_alpha); put(s.contexts); put(s.prefix); };
  for (int64_t x : {(int64_t)n, (int64_t)P.n_extra, (int64_t)P.global_direct, (int64_t)P.lean_mod, (int64_t)P.lane_stride, (int64_t)P.hf_waves,
                    (int64_t)P.alpha_stride, (int64_t)P.per_alpha_wg, (int64_t)P.lf_per_wave, (int64_t)P.mod_lanes, (int64_t)P.mod_rb, (int64_t)P.mod_wp_lds,
                    (int64_t)P.direct_lf, (int64_t)P.direct_alpha, (int64_t)P.direct_mod, (int64_t)P.lf.lds, (int64_t)P.lf.global, (int64_t)P.hf.lds,
                    (int64_t)P.hf.global, (int64_t)P.lds_hf_lanes, (int64_t)P.alpha.lds, (int64_t)P.alpha.global, (int64_t)P.mod.lds, (int64_t)P.mod.global,
                    (int64_t)P.max_mod_groups, (int64_t)P.max_mod_coded})
    put(x);
  for (int i = 0; i < n; i++) {
    const ParsedFrame& f = frames[i];
    const FramePlan& r = P.frames[i];
    for (int64_t x : {(int64_t)status[i], (int64_t)r.decoded, (int64_t)f.encoding, (int64_t)f.single, (int64_t)f.xg, (int64_t)f.yg, (int64_t)f.ng, (int64_t)f.xlf,
                      (int64_t)f.ylf, (int64_t)f.nlf, (int64_t)f.num_passes, (int64_t)(f.alpha_index >= 0), (int64_t)f.ysize, (int64_t)f.tree.size(),
                      (int64_t)f.tree_row_static, (int64_t)f.tree_uses_wp, (int64_t)r.dec_gy0, (int64_t)r.dec_gy1, (int64_t)r.band_y0, (int64_t)r.band_y1,
                      (int64_t)r.lf0, (int64_t)r.lf1, (int64_t)r.hf0, (int64_t)r.hf1, (int64_t)r.alpha0, (int64_t)r.alpha1, (int64_t)r.hf, (int64_t)r.first_extra,
                      (int64_t)r.hf_per_wg, (int64_t)r.hf_table_bytes})
      put(x);
    put_shape(f.mcode);
    put((int64_t)(1 + f.extra_passes.size()));
    put_shape(f.acode);
    for (auto& ep : f.extra_passes) put_shape(ep.acode);
    put((int64_t)f.sec_size.size());
    for (uint32_t s : f.sec_size) put(s);
  }
  for (const std::vector<SectionTask>* t : {&P.lf_finish_tasks, &P.lf_ans_tasks, &P.pass_tasks, &P.alpha_tasks, &P.mod_tasks}) {
    put((int64_t)t->size());
    for (const SectionTask& k : *t) { put(k.image); put(k.first); put(k.count); }
  }
  put((int64_t)P.hf_orders.size());
  for (auto& ho : P.hf_orders) {
    put(ho.image); put(ho.pass); put((int64_t)ho.order.size());
    for (uint32_t g : ho.order) put(g);
  }
  if (v.size() > capacity) return 0;
  memcpy(out, v.data(), v.size() * sizeof(int64_t));
  return v.size();
}

// Parses n files, plans them and lays their batch out twice (batch_layout.h; nothing touches a GPU): measuring, then placing with the blob
// in an ordinary host buffer (host base = device base) and distinct fake bases, never dereferenced, for the zeroed workspace head (region
// 1), the workspace (2), the callers' output buffers (3), the decoder's static tables (4) and the pixel-chunk planes (5).  opts: as jxlhip_selftest_entropy_plan,
// then debug_taps.  No layered files (composites empty); one-group lossy frames go in without the LF pre-pass.  Read-back: what the
// placed DevImages and task tables point at in the blob is compared with the parsed frames and the plan, one comparison per table.
// out, as numbers (returns how many, 0: they do not fit `capacity`):
//   n, n_extra, pixel_chunk, measured blob / zero / ws bytes, where the placing pass ended in each, comparisons and mismatches of the
//   task and hf_order tables, then the toy sequence that places one allocation more than it measured: did it throw, is the guard behind
//   its buffer intact; measured bytes of the pixel-chunk planes, where the placing pass ended in them;
//   the measuring pass's allocation log: count, then (region, offset, bytes, align) each; the placing pass's likewise;
//   per image record (the batch's images, then the later passes' records): image it belongs to, parse status, decoded, are its DevImage
//   bytes all zero, encoding, w, h, w8, h8, ng, nlf, cs_size, region and offset of cs, comparisons, mismatches; count, then (field, region,
//   offset) of every non-null pointer of `fields` below, in its order; count, then (split, msb, lsb, packed cfg word) of every cluster of its
//   codes (images: Modular code, then the first pass's HF code; pass records: their HF code).
extern "C" JXLFILETYPEIO_API size_t jxlhip_selftest_batch_layout(int32_t n, const uint8_t* const* data, const size_t* sizes, const int32_t* opts,
                                                                 int64_t* out, size_t capacity) {
  std::vector<ParsedFrame> frames((size_t)n);
  std::vector<int> status((size_t)n, DecoderStatus_Ok);
  for (int i = 0; i < n; i++) {
    try {
      ParseFile(data[i], sizes[i], false, frames[i]);
    } catch (const std::exception&) {
      status[i] = DecoderStatus_DecodeError;
    }
  }
  EntropyPlanOptions o;
  o.band_first_row = opts[0]; o.band_rows = opts[1]; o.downscale = opts[2]; o.lane_stride_override = opts[3];
  o.no_direct = opts[4] != 0; o.mod_lanes64 = opts[5] != 0;
  const EntropyPlan P = PlanEntropy(frames, status, o);
  const uintptr_t kZero = (uintptr_t)1 << 44, kWs = (uintptr_t)2 << 44, kOut = (uintptr_t)3 << 44, kStatic = (uintptr_t)4 << 44, kPix = (uintptr_t)5 << 44,
                  kSpan = (uintptr_t)1 << 44;
  std::vector<uint8_t*> dev_out((size_t)n);
  for (int i = 0; i < n; i++) dev_out[i] = (uint8_t*)(kOut + ((uintptr_t)i << 34));
  const uint16_t* d_natural[kNumOrders]; const U32x2* d_scan[kNumQuantTables]; const float* d_dq[kNumQuantTables]; uint32_t dq_n[kNumQuantTables];
  for (int k = 0; k < kNumOrders; k++) d_natural[k] = (const uint16_t*)(kStatic + ((uintptr_t)k << 24));
  for (int q = 0; q < kNumQuantTables; q++) {
    d_scan[q] = (const U32x2*)(kStatic + ((uintptr_t)(64 + q) << 24)); d_dq[q] = (const float*)(kStatic + ((uintptr_t)(128 + q) << 24));
    dq_n[q] = (uint32_t)(GetStaticTables().dq[q].size() / 3);
  }
  const std::vector<Composite> comps;
  const std::vector<int> file_of;
  const std::vector<ParsedFrame> files;
  BatchInput in;
  in.frames = &frames; in.parse_status = &status; in.plan = &P;
  in.dev_out = dev_out.data();
  in.comps = &comps; in.file_of = &file_of; in.files = &files; in.nfiles = n;
  in.d_natural = d_natural; in.d_scan = d_scan; in.d_dq = d_dq; in.dq_n = dq_n;
  in.ds = opts[2] == 8; in.debug_taps = opts[6] != 0;
  std::vector<Region::Entry> log_m, log_p;
  BatchRegions M;
  M.blob.id = 0; M.zero.id = 1; M.ws.id = 2; M.pix.id = 5;
  M.blob.log = M.zero.log = M.ws.log = M.pix.log = &log_m;
  {
    BatchOutput unplaced;
    BuildBatch(in, M, unplaced);
  }
  std::vector<uint8_t> blob(M.blob.off + 1, 0);
  BatchRegions R{Region(blob.data(), blob.data(), M.blob.off), Region(nullptr, (const void*)kZero, M.zero.off), Region(nullptr, (const void*)kWs, M.ws.off),
                 Region(nullptr, (const void*)kPix, M.pix.off)};
  R.blob.id = 0; R.zero.id = 1; R.ws.id = 2; R.pix.id = 5;
  R.blob.log = R.zero.log = R.ws.log = R.pix.log = &log_p;
  BatchOutput B;
  BuildBatch(in, R, B);
  std::vector<int64_t> v;
  auto put = [&](int64_t x) { v.push_back(x); };
  const uintptr_t blob0 = (uintptr_t)blob.data();
  auto region_of = [&](const void* p, int64_t* off) {
    const uintptr_t a = (uintptr_t)p;
    if (a >= blob0 && a < blob0 + M.blob.off) { *off = (int64_t)(a - blob0); return 0; }
    const uintptr_t bases[5] = {kZero, kWs, kOut, kStatic, kPix};
    for (int k = 0; k < 5; k++) if (a >= bases[k] && a < bases[k] + kSpan) { *off = (int64_t)(a - bases[k]); return k + 1; }
    *off = 0;
    return -1;
  };
  // one comparison: `bytes` at p, which must lie in the blob, equal `want` (null: only where they lie is checked)
  int64_t cmp = 0, bad = 0;
  auto same = [&](const void* p, const void* want, size_t bytes) {
    cmp++;
    const uintptr_t a = (uintptr_t)p;
    if (a < blob0 || a > blob0 + M.blob.off || bytes > blob0 + M.blob.off - a || (bytes && want && memcmp(p, want, bytes))) bad++;
  };
  auto same_code = [&](const DevCode& dc, const HostCode& hc, std::vector<int64_t>& cfg) {
    same(dc.ctx_map, hc.ctx_map.data(), hc.ctx_map.size());
    same(dc.alias, hc.alias.data(), 8 * hc.alias.size());
    cmp++;
    if (dc.num_ctx != hc.ctx_map.size() || dc.num_clusters != hc.num_hist || dc.log_alpha != hc.log_alpha) bad++;
    same(dc.cfg, nullptr, 4 * hc.cfg.size());   // in the blob; the test checks the words
    for (size_t k = 0; k < hc.cfg.size(); k++) { cfg.push_back(hc.cfg[k].split); cfg.push_back(hc.cfg[k].msb); cfg.push_back(hc.cfg[k].lsb); cfg.push_back(dc.cfg[k]); }
    if (hc.use_prefix) {
      size_t at = 0;
      for (size_t k = 0; k < hc.prefix.size(); k++) {
        same(dc.pfx_count + 16 * k, hc.prefix[k].count, 32);
        const uint32_t off = (uint32_t)at;
        same(dc.pfx_off + k, &off, 4);
        same(dc.pfx_sorted + at, hc.prefix[k].sorted.data(), 2 * hc.prefix[k].sorted.size());
        at += hc.prefix[k].sorted.size();
      }
    }
  };
  auto same_tasks = [&](const SectionTask* t, const std::vector<SectionTask>& want) { same(t, want.data(), sizeof(SectionTask) * want.size()); };
  same_tasks(B.lf_tasks, P.lf_finish_tasks); same_tasks(B.pass_tasks, P.pass_tasks); same_tasks(B.lf_ans_tasks, P.lf_ans_tasks);
  same_tasks(B.mod_tasks, P.mod_tasks); same_tasks(B.alpha_tasks, P.alpha_tasks);
  for (const EntropyPlan::HfOrder& ho : P.hf_orders)
    same(B.imgs[ho.pass ? (size_t)P.frames[ho.image].first_extra + ho.pass - 1 : (size_t)ho.image].hf_order, ho.order.data(), 4 * ho.order.size());
  same(B.d_imgs, B.imgs.data(), sizeof(DevImage) * B.imgs.size());
  // the toy sequence: two allocations measured, three placed
  int64_t threw = 0, guard_ok = 1;
  {
    Region m;
    m.Take(100); m.Take(50);
    std::vector<uint8_t> buf(m.off + 64, 0xA5);
    Region r(buf.data(), buf.data(), m.off);
    const std::vector<uint8_t> src(100, 0x11);
    try {
      r.Put(src.data(), 100); r.Put(src.data(), 50); r.Put(src.data(), 8);
    } catch (const std::length_error&) {
      threw = 1;
    }
    for (size_t k = m.off; k < buf.size(); k++) if (buf[k] != 0xA5) guard_ok = 0;
  }
  for (int64_t x : {(int64_t)n, (int64_t)P.n_extra, (int64_t)B.pixel_chunk, (int64_t)M.blob.off, (int64_t)M.zero.off, (int64_t)M.ws.off, (int64_t)R.blob.off,
                    (int64_t)R.zero.off, (int64_t)R.ws.off, cmp, bad, threw, guard_ok, (int64_t)M.pix.off, (int64_t)R.pix.off})
    put(x);
  for (const std::vector<Region::Entry>* log : {&log_m, &log_p}) {
    put((int64_t)log->size());
    for (const Region::Entry& e : *log) { put(e.region); put((int64_t)e.off); put((int64_t)e.bytes); put((int64_t)e.align); }
  }
  std::vector<int> image_of(B.imgs.size(), -1);
  for (int i = 0; i < n; i++) {
    image_of[i] = i;
    if (status[i] == DecoderStatus_Ok && frames[i].encoding == 0)
      for (size_t p = 0; p < frames[i].extra_passes.size(); p++) image_of[(size_t)P.frames[i].first_extra + p] = i;
  }
  for (size_t r = 0; r < B.imgs.size(); r++) {
    const DevImage& d = B.imgs[r];
    const int i = image_of[r];
    const ParsedFrame& f = frames[i];
    const bool decoded = status[i] == DecoderStatus_Ok;
    bool all_zero = true;
    for (size_t k = 0; k < sizeof(DevImage); k++) all_zero &= ((const uint8_t*)&d)[k] == 0;
    cmp = bad = 0;
    std::vector<int64_t> cfg;
    if (decoded) {
      same(d.cs, f.cs, f.cs_size);
      same(d.sec_off, f.sec_off.data(), 8 * f.sec_off.size());
      same(d.sec_size, f.sec_size.data(), 4 * f.sec_size.size());
      same(d.tree, f.tree.data(), sizeof(DevTreeNode) * f.tree.size());
      if ((int)r < n) same_code(d.mcode, f.mcode, cfg);
      if (f.encoding == 0) {
        const size_t pass = (int)r < n ? 0 : r - (size_t)P.frames[i].first_extra + 1;
        same_code(d.acode, pass ? f.extra_passes[pass - 1].acode : f.acode, cfg);
        for (int ob = 0; ob < kNumOrders; ob++)
          for (int c = 0; c < 3; c++) {
            const std::vector<uint16_t>& own = f.custom_order[ob][c];
            if (!own.empty()) same(d.order[ob * 3 + c], own.data(), 2 * own.size());
            else { cmp++; if (d.order[ob * 3 + c] != d_natural[ob]) bad++; }
          }
      }
    }
    int64_t cs_off = 0;
    const int cs_region = region_of(d.cs, &cs_off);
    for (int64_t x : {(int64_t)i, (int64_t)status[i], (int64_t)decoded, (int64_t)all_zero, (int64_t)f.encoding, (int64_t)f.xsize, (int64_t)f.ysize, (int64_t)f.w8,
                      (int64_t)f.h8, (int64_t)f.ng, (int64_t)f.nlf, (int64_t)f.cs_size, (int64_t)cs_region, cs_off, cmp, bad})
      put(x);
    // every pointer of a DevImage into the workspace (or, for `out`, the caller's buffer), in the order of
    // tests/test_batch_layout.py's FIELDS
    const void* const fields[] = {
        d.lf[0], d.lf[1], d.lf[2], d.lf_tmp[0], d.lf_tmp[1], d.lf_tmp[2], d.lf_final[0], d.lf_final[1], d.lf_final[2], d.lfq[0], d.lfq[1], d.lfq[2],
        d.lf_extra, d.cellinfo, d.rawq, d.sharp, d.ytox, d.ytob, d.binfo, d.lf_desc, d.lf_count, d.alpha_desc, d.blk_list, d.blk_count, d.grp_bitpos,
        d.alpha_bitpos, d.lf_end_bits, d.mod_plane[0], d.mod_plane[1], d.mod_plane[2], d.mod_plane[3], d.mod_plane[4], d.mod_desc, d.wp_lf, d.wp_grp,
        d.lz_lf, d.lz_grp, d.lz_hf, d.lz_mod, d.alpha32, d.centries, d.cblk, d.coef[0], d.coef[1], d.coef[2], d.tmp[0], d.tmp[1], d.tmp[2], d.xyb[0],
        d.xyb[1], d.xyb[2], d.xyb2[0], d.xyb2[1], d.xyb2[2], d.inv_sigma, d.tile_list, d.alpha, d.out, d.status, d.noise_rnd[0], d.noise_rnd[1],
        d.noise_rnd[2], d.noise[0], d.noise[1], d.noise[2], d.ds_alpha, d.ds_out};
    std::vector<int64_t> fl;
    for (size_t k = 0; k < sizeof(fields) / sizeof(fields[0]); k++) {
      if (!fields[k]) continue;
      int64_t off = 0;
      const int reg = region_of(fields[k], &off);
      fl.push_back((int64_t)k); fl.push_back(reg); fl.push_back(off);
    }
    put((int64_t)fl.size() / 3);
    for (int64_t x : fl) put(x);
    put((int64_t)cfg.size() / 4);
    for (int64_t x : cfg) put(x);
  }
  if (v.size() > capacity) return 0;
  memcpy(out, v.data(), v.size() * sizeof(int64_t));
  return v.size();
}

// ---- the varblock rules (csrc/varblock_rules.h) and recon_tile_kernel's LDS layout, as the kernels and the host call them;
// tests/test_varblock_rules.py holds each against a statement written out in Python.
// Per strategy id, six numbers: valid, log2 cx, log2 cy, order bucket, quant table, special | afv << 1 (ids outside the tables: valid alone).
extern "C" JXLFILETYPEIO_API void jxlhip_selftest_varblock_strategy(int32_t s, int32_t* out) {
  for (int k = 0; k < 6; k++) out[k] = 0;
  out[0] = StrategyValid(s) ? 1 : 0;
  if (!out[0]) return;
  out[1] = StrategyLog2Cx(s); out[2] = StrategyLog2Cy(s); out[3] = (int32_t)StrategyOrderBucket(s); out[4] = (int32_t)StrategyQuantTable(s);
  out[5] = (StrategyIsSpecial(s) ? 1 : 0) | (StrategyIsAfv(s) ? 2 : 0);
}
extern "C" JXLFILETYPEIO_API uint32_t jxlhip_selftest_varblock_cell_pack(uint32_t s, uint32_t ix, uint32_t iy, uint32_t lcx, uint32_t lcy) {
  return CellInfoPack(s, ix, iy, lcx, lcy);
}
// strategy, ix, iy, log2 cx, log2 cy, valid, origin
extern "C" JXLFILETYPEIO_API void jxlhip_selftest_varblock_cell_unpack(uint32_t info, uint32_t* out) {
  out[0] = CellStrategy(info); out[1] = CellIx(info); out[2] = CellIy(info); out[3] = CellLog2Cx(info); out[4] = CellLog2Cy(info);
  out[5] = CellValid(info) ? 1 : 0; out[6] = CellIsOrigin(info) ? 1 : 0;
}
// The stored layout of a block of 8 << lcy rows and 8 << lcx columns, row-major over (ky, kx): StoredIndex, what StoredToKyKx makes of
// that index (ky << 16 | kx) and IsLlfPosition.  meta: log2 of the pitch, transposed.
extern "C" JXLFILETYPEIO_API void jxlhip_selftest_varblock_stored(int32_t special, uint32_t lcx, uint32_t lcy, uint32_t* meta, uint32_t* index,
                                                                  uint32_t* back, uint8_t* llf) {
  const uint32_t lng = StoredLog2Pitch(lcx, lcy);
  const bool transposed = StoredTransposed(special != 0, lcx, lcy);
  meta[0] = lng; meta[1] = transposed ? 1 : 0;
  const uint32_t R = 8u << lcy, C = 8u << lcx;
  for (uint32_t ky = 0; ky < R; ky++)
    for (uint32_t kx = 0; kx < C; kx++) {
      const uint32_t p = StoredIndex(ky, kx, lng, transposed);
      uint32_t by, bx;
      StoredToKyKx(p, lng, transposed, &by, &bx);
      index[ky * C + kx] = p; back[ky * C + kx] = by << 16 | bx; llf[ky * C + kx] = IsLlfPosition(ky, kx, lcx, lcy) ? 1 : 0;
    }
}
extern "C" JXLFILETYPEIO_API int32_t jxlhip_selftest_varblock_basis_offset(int32_t small, int32_t n) { return small ? BasisSmallOffset(n) : BasisAllOffset(n); }
extern "C" JXLFILETYPEIO_API int32_t jxlhip_selftest_varblock_channel_of_team(int32_t i) { return ChannelOfTeam(i); }
// form 0: the quotient by division; 1: through a reciprocal (1.0f / f on the host)
extern "C" JXLFILETYPEIO_API float jxlhip_selftest_varblock_dequant_bias(int32_t v, float qb, float qb3, int32_t form) {
  if (form == 0) return DequantBias(v, qb, qb3, ExactQuotient());
  return DequantBias(v, qb, qb3, [](float a, float f) { return a * (1.0f / f); });
}
// recon_tile_kernel's LDS (lds_layout.h): the offsets in layout order, then `end`; returns how many numbers
extern "C" JXLFILETYPEIO_API int32_t jxlhip_selftest_varblock_recon_lds(int64_t* out) {
  const ReconTileLds l;
  const size_t v[14] = {l.cfc3, l.B816, l.cscale, l.ci, l.cmeta, l.cnq, l.cpre, l.cstart, l.ctot, l.csc, l.t32_lo, l.t32_hi, l.t64, l.end};
  for (int k = 0; k < 14; k++) out[k] = (int64_t)v[k];
  return 14;
}

// ---- the Modular sample rules (csrc/modular_rules.h), as the kernels and the host encoder call them; tests/test_modular_rules.py
// holds each against the format's definition.  Neighbourhoods travel as rows of seven int32: W, N, NW, NE, NN, WW, NEE.
extern "C" JXLFILETYPEIO_API uint32_t jxlhip_selftest_pack_signed(int32_t v) { return PackSigned(v); }
extern "C" JXLFILETYPEIO_API int32_t jxlhip_selftest_unpack_signed(uint32_t u) { return UnpackSigned(u); }

namespace {
template <int kPred>
void PredictAllT(const int32_t* h, int64_t wp, int32_t* out) {
  out[kPred] = (int32_t)ModularPredictT<kPred>(h[0], h[1], h[2], h[3], h[4], h[5], h[6], wp);
  if constexpr (kPred < 13) PredictAllT<kPred + 1>(h, wp, out);
}
}  // namespace

// Per neighbourhood: the low 32 bits of predictors 0 .. 13 by the run-time id (by_id) and by the compile-time id (by_template),
// ClampedGradient32, and RowGuess for the ids 0, 1, 2 and 5.
extern "C" JXLFILETYPEIO_API void jxlhip_selftest_modular_predict(int32_t n, const int32_t* hoods, const int64_t* wp_pred, int32_t* by_id,
                                                                  int32_t* by_template, int32_t* gradient32, uint32_t* row_guess) {
  for (int i = 0; i < n; i++) {
    const int32_t* h = hoods + 7 * (size_t)i;
    for (uint32_t p = 0; p < 14; p++) by_id[14 * (size_t)i + p] = (int32_t)ModularPredict(p, h[0], h[1], h[2], h[3], h[4], h[5], h[6], wp_pred[i]);
    PredictAllT<0>(h, wp_pred[i], by_template + 14 * (size_t)i);
    gradient32[i] = ClampedGradient32(h[0], h[1], h[2]);
    const uint32_t ids[4] = {0, 1, 2, 5};
    for (int k = 0; k < 4; k++) row_guess[4 * (size_t)i + k] = RowGuess(ids[k], h[0], h[1], h[2]);
  }
}

// Per (W, N, NW): ClampedGradientSmall and ClampedGradient32
extern "C" JXLFILETYPEIO_API void jxlhip_selftest_gradient_small(int32_t n, const int32_t* wnnw, int32_t* small, int32_t* gradient32) {
  for (int i = 0; i < n; i++) {
    const int32_t* h = wnnw + 3 * (size_t)i;
    small[i] = ClampedGradientSmall(h[0], h[1], h[2]);
    gradient32[i] = ClampedGradient32(h[0], h[1], h[2]);
  }
}

// Per neighbourhood (with prev9, wp_err and x, y of its own): properties 2 .. 15, out[14 * i + id - 2]
extern "C" JXLFILETYPEIO_API void jxlhip_selftest_modular_property(int32_t n, const int32_t* hoods, const int64_t* prev9, const int64_t* wp_err,
                                                                   const int32_t* xy, int64_t* out) {
  for (int i = 0; i < n; i++) {
    const int32_t* h = hoods + 7 * (size_t)i;
    ModularHood hd;
    hd.W = h[0]; hd.N = h[1]; hd.NW = h[2]; hd.NE = h[3]; hd.NN = h[4]; hd.WW = h[5]; hd.NEE = h[6];
    hd.prev9 = prev9[i]; hd.wp_err = wp_err[i]; hd.x = xy[2 * i]; hd.y = xy[2 * i + 1];
    for (int id = 2; id < 16; id++) out[14 * (size_t)i + id - 2] = ModularProperty(id, hd);
  }
}
// The linear form of property `id`: coefficients over W, N, NW, NE, NN, WW, x, y, wp_err, then the abs and the minus-prev9 flags
extern "C" JXLFILETYPEIO_API void jxlhip_selftest_modular_property_form(int32_t id, int32_t* out) {
  const PropertyForm f = ModularPropertyForm(id);
  const int32_t v[11] = {f.cW, f.cN, f.cNW, f.cNE, f.cNN, f.cWW, f.cX, f.cY, f.cE, f.abs ? 1 : 0, f.minus_prev9 ? 1 : 0};
  memcpy(out, v, sizeof(v));
}

// The neighbourhood and prev9 of every sample of a w x h image as a decode loop carries it (ModularRoll, HasNE / HasNN / HasNEE);
// by_roll == 0: W, N and NW by position instead (ModularWNNWAt), the rest as before.
extern "C" JXLFILETYPEIO_API void jxlhip_selftest_modular_hoods(int32_t w, int32_t h, const int32_t* img, int32_t by_roll, int32_t* hoods,
                                                                int64_t* prev9) {
  const auto at = [&](int x, int y) { return img[(size_t)y * w + x]; };
  for (int y = 0; y < h; y++) {
    ModularRoll r;
    r.StartRow(y ? at(0, y - 1) : 0);
    for (int x = 0; x < w; x++) {
      int32_t* o = hoods + 7 * ((size_t)y * w + x);
      const int32_t NE = HasNE(x, y, w) ? at(x + 1, y - 1) : r.N;
      o[0] = r.W; o[1] = r.N; o[2] = r.NW; o[3] = NE; o[4] = HasNN(y) ? at(x, y - 2) : r.N; o[5] = r.WW;
      o[6] = HasNEE(x, y, w) ? at(x + 2, y - 1) : NE;
      prev9[(size_t)y * w + x] = r.prev9;
      if (!by_roll) { const ModularWNNW p = ModularWNNWAt(at, x, y); o[0] = p.W; o[1] = p.N; o[2] = p.NW; }
      r.Step(at(x, y), NE, x, y);
    }
  }
}

// -1 when a token under configuration word `cfg` has to be read from the stream, else the symbol it is known to be
extern "C" JXLFILETYPEIO_API int32_t jxlhip_selftest_one_symbol_token(uint32_t cfg) { return OneSymbolToken(cfg) ? (int32_t)OneSymbol(cfg) : -1; }
extern "C" JXLFILETYPEIO_API uint32_t jxlhip_selftest_leaf_residual(uint32_t u, uint32_t mul, uint32_t off) { return LeafResidual(u, mul, off); }

// StaticWalk over `count` nodes of (property, splitval, a, b) from the root: the index of the node it ends in; out[0] = whether the
// row was looked at, out[1] / out[2] = LeafPredictor / LeafContext of that node.  with_row = 0: channel and stream only.
extern "C" JXLFILETYPEIO_API int32_t jxlhip_selftest_static_walk(const int32_t* nodes, int32_t count, int32_t chan, int32_t sid, int32_t y,
                                                                 int32_t with_row, int32_t* out) {
  const auto node_at = [&](uint32_t i) {
    DevTreeNode nd{-1, 0, 0, 0};
    if (i < (uint32_t)count) { nd.property = nodes[4 * i]; nd.splitval = nodes[4 * i + 1]; nd.a = (uint32_t)nodes[4 * i + 2]; nd.b = (uint32_t)nodes[4 * i + 3]; }
    return nd;
  };
  DevTreeNode nd;
  bool used_y = false;
  const uint32_t at = with_row ? StaticWalk<true>(node_at, 0u, chan, sid, y, &used_y, &nd) : StaticWalk<false>(node_at, 0u, chan, sid, y, &used_y, &nd);
  out[0] = used_y ? 1 : 0; out[1] = (int32_t)LeafPredictor(nd); out[2] = (int32_t)LeafContext(nd);
  return (int32_t)at;
}

// The weighted predictor over a whole image, state in the memory form (WpState, as ModularChannel keeps it): per sample the
// predictor-6 guess and property 15.
extern "C" JXLFILETYPEIO_API void jxlhip_selftest_wp(int32_t w, int32_t h, const int32_t* img, int64_t* guess, int64_t* max_err) {
  std::vector<int32_t> scratch((size_t)WpState::kInts * (w + 2));
  WpState wp;
  wp.Init(scratch.data(), w);
  const auto at = [&](int x, int y) { return img[(size_t)y * w + x]; };
  for (int y = 0; y < h; y++) {
    ModularRoll r;
    r.StartRow(y ? at(0, y - 1) : 0);
    for (int x = 0; x < w; x++) {
      const int32_t NE = HasNE(x, y, w) ? at(x + 1, y - 1) : r.N;
      guess[(size_t)y * w + x] = wp.Predict(x, y, w, r.N, r.W, NE, &max_err[(size_t)y * w + x]);
      wp.Update(at(x, y), x, y);
      r.Step(at(x, y), NE, x, y);
    }
  }
}

// ---- the workspace of a batch encode (csrc/enc_batch_layout.cc: LayEncBatch), measured and then placed at a made-up base.
// items: 6 int32 per image (w, h, channels, bytes per sample, lossless, fitted chroma-from-luma maps).  out (int64 each; returns how many the full answer takes):
//   n; total bytes measured; total bytes placed; head bytes; the four region bounds; tables, records_m, mcodes, records_a, acodes, dst_off,
//   body; total sections; sizeof(EncImage); kEncModCodeBytes; kEncHfCodeBytes; then per image: begin, end, src, surface, sections, count,
//   and per non-null buffer pointer of its EncImage (in the order of `fields` below) the field's number, the offset the measuring pass
//   gave it and the offset the placing pass gave it.
extern "C" JXLFILETYPEIO_API size_t jxlhip_selftest_enc_batch_layout(int32_t n, const int32_t* items, int64_t* out, size_t capacity) {
  std::vector<EncBatchItem> it((size_t)n);
  for (int i = 0; i < n; i++)
    it[i] = EncBatchItem{(uint32_t)items[6 * i], (uint32_t)items[6 * i + 1], items[6 * i + 2], items[6 * i + 3], items[6 * i + 4], items[6 * i + 5]};
  std::vector<EncImage> a((size_t)n), b((size_t)n);
  EncBatchLayout la, lb;
  uint8_t* const base = (uint8_t*)((uintptr_t)2 << 44);
  LayEncBatch(it.data(), n, nullptr, a.data(), &la);
  LayEncBatch(it.data(), n, base, b.data(), &lb);
  std::vector<int64_t> v;
  v.push_back(n); v.push_back((int64_t)la.total_bytes); v.push_back((int64_t)lb.total_bytes); v.push_back((int64_t)lb.head_bytes);
  for (int k = 0; k <= kNumEncCounterKinds; k++) v.push_back((int64_t)lb.region[k]);
  for (size_t x : {lb.tables, lb.records_m, lb.mcodes, lb.records_a, lb.acodes, lb.dst_off, lb.body, lb.total_sections, sizeof(EncImage),
                   kEncModCodeBytes, kEncHfCodeBytes}) v.push_back((int64_t)x);
  auto fields = [](const EncImage& im) {
    std::vector<const void*> f;
    for (int c = 0; c < 3; c++) f.push_back(im.xyb[c]);
    for (int c = 0; c < 3; c++) f.push_back(im.pad[c]);
    f.push_back(im.alpha_px);
    for (int c = 0; c < 3; c++) f.push_back(im.lfq[c]);
    f.push_back(im.rawq); f.push_back(im.act); f.push_back(im.strat);
    for (int c = 0; c < 3; c++) f.push_back(im.qs[c]);
    for (int c = 0; c < 3; c++) f.push_back(im.nz[c]);
    for (int c = 0; c < 3; c++) f.push_back(im.nzc[c]);
    for (int c = 0; c < 3; c++) f.push_back(im.last[c]);
    f.push_back(im.tok_lf); f.push_back(im.tok_meta); f.push_back(im.tok_ac); f.push_back(im.tok_alpha);
    f.push_back(im.n_ac); f.push_back(im.n_meta); f.push_back(im.hist_mod); f.push_back(im.hist_ac);
    for (int c = 0; c < 4; c++) f.push_back(im.ll_plane[c]);
    f.push_back(im.tok_ll); f.push_back(im.sec_bytes); f.push_back(im.stream_state); f.push_back(im.sec_bits);
    return f;
  };
  for (int i = 0; i < n; i++) {
    const EncBatchSlot& sl = lb.slots[(size_t)i];
    v.push_back((int64_t)sl.begin); v.push_back((int64_t)sl.end); v.push_back((int64_t)sl.src); v.push_back((int64_t)sl.surface);
    v.push_back(EncNumSections(b[i]));
    const std::vector<const void*> fa = fields(a[i]), fb = fields(b[i]);
    const size_t at = v.size();
    v.push_back(0);
    for (size_t k = 0; k < fb.size(); k++) {
      if (!fb[k]) continue;
      v.push_back((int64_t)k); v.push_back((int64_t)(uintptr_t)fa[k]); v.push_back((int64_t)((uintptr_t)fb[k] - (uintptr_t)base));
      v[at]++;
    }
  }
  if (out) memcpy(out, v.data(), std::min(capacity, v.size()) * sizeof(int64_t));
  return v.size();
}

// The plan of an animation decode, without a GPU (host_parse.h: ParseAnimation, animation.h).  counts[0 .. ncounts): the `count` of
// successive jxlhip_animation_next calls (<= 0: all that is left).  scratch_budget: bytes of scratch a chunk may take (<= 0: the
// decoder's kAnimChunkScratch).  out, as numbers (returns how many; 0: refused - *status and err say
// why - or they do not fit `capacity`):
//   frames, displayed images, have_animation, tps_numerator, tps_denominator, num_loops, have_timecodes, raw, canvas width, canvas height, is the file one
//   single-frame image;
//   per frame: displayed image it completes (-1), duration, timecode, save slot (-1), mask of the slots it reads, source and mode of the
//   colour channels, source and mode of the alpha channel, is its crop smaller than the canvas, its scratch bytes, the slots alive
//   behind it, the length of its name and the name's bytes;
//   chunks, then per chunk: the call it belongs to, first frame, frames, first displayed image, displayed images, live_in, live_out.
extern "C" JXLFILETYPEIO_API size_t jxlhip_selftest_animation_plan(const uint8_t* data, size_t size, int32_t chunk_frames, int64_t scratch_budget,
                                                                   const int32_t* counts, int32_t ncounts, int64_t* out, size_t capacity, int32_t* status, ErrorInfo* err) {
  if (status) *status = DecoderStatus_Ok;
  try {
    Animation a;
    ParseAnimation(data, size, false, a);
    const AnimPlan p = PlanAnimation(a);
    std::vector<int64_t> v;
    auto put = [&](int64_t x) { v.push_back(x); };
    const ParsedFrame& h = a.head;
    for (int64_t x : {(int64_t)a.frames.size(), (int64_t)a.completes.size(), (int64_t)h.have_animation, (int64_t)h.tps_numerator, (int64_t)h.tps_denominator,
                      (int64_t)h.num_loops, (int64_t)h.have_timecodes, (int64_t)a.raw, (int64_t)h.xsize, (int64_t)h.ysize, (int64_t)a.single})
      put(x);
    for (size_t k = 0; k < a.frames.size(); k++) {
      const ParsedFrame& f = a.frames[k];
      const BlendInfo& bc = f.blend[0];
      const BlendInfo& ba = f.alpha_index >= 0 ? f.blend[1 + f.alpha_index] : bc;
      const bool partial = f.have_crop && !(f.crop_x0 <= 0 && f.crop_y0 <= 0 && f.crop_x0 + (int64_t)f.xsize >= h.xsize && f.crop_y0 + (int64_t)f.ysize >= h.ysize);
      for (int64_t x : {(int64_t)a.show[k], (int64_t)f.duration, (int64_t)f.timecode, (int64_t)a.save[k], (int64_t)SlotsRead(f, h.xsize, h.ysize), (int64_t)bc.source,
                        (int64_t)bc.mode, (int64_t)ba.source, (int64_t)ba.mode, (int64_t)partial, (int64_t)p.scratch[k], (int64_t)p.live_after[k], (int64_t)f.name.size()})
        put(x);
      for (char c : f.name) put((uint8_t)c);
    }
    const size_t nchunks_at = v.size();
    put(0);
    int next_frame = 0, next_shown = 0, nchunks = 0;
    const int total = (int)a.completes.size();
    for (int call = 0; call < ncounts; call++) {
      const int n = counts[call] <= 0 ? total - next_shown : std::min(counts[call], total - next_shown);
      const int last = next_shown + n - 1;
      while (next_shown <= last) {
        const AnimChunk c = NextChunk(a, p, next_frame, last, chunk_frames, scratch_budget > 0 ? (size_t)scratch_budget : kAnimChunkScratch);
        for (int64_t x : {(int64_t)call, (int64_t)c.first, (int64_t)c.count, (int64_t)c.first_shown, (int64_t)c.shown, (int64_t)c.live_in, (int64_t)c.live_out}) put(x);
        next_frame += c.count; next_shown += c.shown; nchunks++;
      }
    }
    v[nchunks_at] = nchunks;
    if (v.size() > capacity) return 0;
    memcpy(out, v.data(), v.size() * sizeof(int64_t));
    return v.size();
  } catch (const ParseError& e) {
    if (status) *status = e.status;
    SetEncErr(err, e.what());
  } catch (const std::exception& e) {
    if (status) *status = DecoderStatus_DecodeError;
    SetEncErr(err, e.what());
  }
  return 0;
}

// Seeking and thumbnails of an animation decode, without a GPU: the host logic of jxlhip_animation_seek / _next / _next_reduced
// (animation.h: EntryPoints, SeekCursor, DeliverImages) run over a list of operations.  ops: nops triples (kind, a, b) - 0: seek a;
// 1: next a (a <= 0: all that is left); 2: next_reduced a b (a <= 0: all that is left, b: the step).  chunk_frames, scratch_budget: as
// jxlhip_selftest_animation_plan.  out, as numbers (returns how many; 0: the file is refused or they do not fit):
//   entry points, then each of them;
//   per operation: 1 (0: refused - a seek outside the file, a step < 1; nothing moved), and the position behind it: codestream frame,
//   displayed image;
//   chunks, then per chunk: the operation it belongs to, first frame, frames, first displayed image, displayed images, live_in, live_out,
//   first stored image (-1: none), stored images, step (the chunk stores first stored + i * step).
extern "C" JXLFILETYPEIO_API size_t jxlhip_selftest_animation_seek_plan(const uint8_t* data, size_t size, int32_t chunk_frames, int64_t scratch_budget,
                                                                        const int32_t* ops, int32_t nops, int64_t* out, size_t capacity, int32_t* status,
                                                                        ErrorInfo* err) {
  if (status) *status = DecoderStatus_Ok;
  try {
    Animation a;
    ParseAnimation(data, size, false, a);
    const AnimPlan p = PlanAnimation(a);
    const std::vector<int> entries = EntryPoints(a, p);
    std::vector<int64_t> v, chunks;
    v.push_back((int64_t)entries.size());
    for (int e : entries) v.push_back(e);
    AnimCursor cur;
    int nchunks = 0;
    const size_t budget = scratch_budget > 0 ? (size_t)scratch_budget : kAnimChunkScratch;
    for (int op = 0; op < nops; op++) {
      const int kind = ops[3 * op], x = ops[3 * op + 1], y = ops[3 * op + 2];
      bool ok = true;
      if (kind == 0) {
        ok = SeekCursor(a, entries, cur, x);
      } else {
        const int step = kind == 2 ? y : 1;
        ok = step >= 1;
        if (ok) {
          const int n = SelectedImages(a, cur, x <= 0 ? (int)a.completes.size() : x, step);
          DeliverImages(a, p, cur, n, step, chunk_frames, budget, [&](const AnimChunk& c, int) {
            for (int64_t q : {(int64_t)op, (int64_t)c.first, (int64_t)c.count, (int64_t)c.first_shown, (int64_t)c.shown, (int64_t)c.live_in, (int64_t)c.live_out,
                              (int64_t)c.first_stored, (int64_t)c.stored, (int64_t)c.step})
              chunks.push_back(q);
            nchunks++;
            return true;
          });
        }
      }
      for (int64_t q : {(int64_t)ok, (int64_t)cur.frame, (int64_t)cur.shown}) v.push_back(q);
    }
    v.push_back(nchunks);
    v.insert(v.end(), chunks.begin(), chunks.end());
    if (v.size() > capacity) return 0;
    memcpy(out, v.data(), v.size() * sizeof(int64_t));
    return v.size();
  } catch (const ParseError& e) {
    if (status) *status = e.status;
    SetEncErr(err, e.what());
  } catch (const std::exception& e) {
    if (status) *status = DecoderStatus_DecodeError;
    SetEncErr(err, e.what());
  }
  return 0;
}

// ---- animation encode (enc_animation.h, host_write.h): headers and geometry rules, host only

// A bare codestream of the image header and one frame header as the encoder writes them, then the first bit of a TOC (not permuted)
// and the padding to a byte.  in[0..20]: xsize, ysize, gray, alpha, lossless, have_animation, tps_numerator, tps_denominator,
// num_loops, have_crop, x0, y0, crop width, crop height, duration, is_last, save_as_reference, source, bits, exp_bits, epf_iters.
// With have_animation = have_crop = 0, is_last = 1 and the rest of the placement 0 these are the fields' defaults.
extern "C" JXLFILETYPEIO_API size_t jxlhip_selftest_animation_headers(const int64_t* in, uint8_t* dst, size_t capacity) {
  try {
    EncImageInfo ii;
    ii.xsize = (uint32_t)in[0]; ii.ysize = (uint32_t)in[1]; ii.gray = in[2] != 0; ii.alpha = in[3] != 0; ii.xyb = !in[4];
    ii.bits = (uint32_t)in[18]; ii.exp_bits = (uint32_t)in[19];
    if (in[5]) { ii.have_animation = true; ii.tps_numerator = (uint32_t)in[6]; ii.tps_denominator = (uint32_t)in[7]; ii.num_loops = (uint32_t)in[8]; }
    EncFrameInfo fi;
    fi.encoding = in[4] ? 1 : 0;
    fi.gab = !in[4]; fi.epf_iters = in[4] ? 0 : (uint32_t)in[20];
    fi.at.have_crop = in[9] != 0;
    fi.at.x0 = (int32_t)in[10]; fi.at.y0 = (int32_t)in[11]; fi.at.width = (uint32_t)in[12]; fi.at.height = (uint32_t)in[13];
    fi.at.duration = (uint32_t)in[14]; fi.at.is_last = in[15] != 0; fi.at.save_as_reference = (uint32_t)in[16]; fi.at.source = (uint32_t)in[17];
    BitWriter cs;
    WriteCodestreamHeaders(ii, cs);
    WriteFrameHeader(ii, fi, cs);
    cs.Bool(false);
    std::vector<uint8_t> bytes = cs.Finish();
    if (bytes.size() > capacity) return 0;
    memcpy(dst, bytes.data(), bytes.size());
    return bytes.size();
  } catch (...) {
    return 0;
  }
}

// The rectangles and placements of n frames on a w x h canvas.  extents: 4 ints (x0, y0, x1, y1; inclusive; x1 < 0: nothing changed)
// per pair, n - 1 of them.  out, 9 ints per frame: x, y, width, height, have_crop, duration, is_last, save_as_reference, source.
extern "C" JXLFILETYPEIO_API void jxlhip_selftest_animation_rects(int32_t n, const int32_t* extents, const uint32_t* durations, int32_t w, int32_t h,
                                                                  int32_t lossless, int32_t key_interval, int32_t* out) {
  for (int32_t k = 0; k < n; k++) {
    const AnimExtent e = k ? AnimExtent{extents[4 * (k - 1)], extents[4 * (k - 1) + 1], extents[4 * (k - 1) + 2], extents[4 * (k - 1) + 3]} : AnimExtent{-1, -1, -1, -1};
    const AnimRect r = AnimFrameRect(k, key_interval, e, w, h, lossless != 0);
    const EncFramePlacement at = AnimPlacement(k, n, r, w, h, durations[k]);
    int32_t* o = out + 9 * k;
    o[0] = r.x; o[1] = r.y; o[2] = r.w; o[3] = r.h;
    o[4] = at.have_crop; o[5] = (int32_t)at.duration; o[6] = at.is_last; o[7] = (int32_t)at.save_as_reference; o[8] = (int32_t)at.source;
    if (at.have_crop && (at.x0 != r.x || at.y0 != r.y || (int32_t)at.width != r.w || (int32_t)at.height != r.h)) o[4] = -1;
  }
}

// AnimFrameRects on the caller's tile table (AnimTilesAcross(w) x AnimTilesAcross(h) words, row-major).  out: x, y, width, height per
// rectangle, up to `capacity` rectangles; returns how many the rule gives.
extern "C" JXLFILETYPEIO_API int32_t jxlhip_selftest_animation_frame_rects(const uint32_t* tiles, int32_t w, int32_t h, int32_t lossless, int32_t max_rects,
                                                                           int32_t merge_pixels, int32_t* out, int32_t capacity) {
  const std::vector<AnimRect> rects = AnimFrameRects(tiles, w, h, lossless != 0, max_rects, merge_pixels);
  for (size_t i = 0; i < rects.size() && (int32_t)i < capacity; i++) {
    out[4 * i] = rects[i].x; out[4 * i + 1] = rects[i].y; out[4 * i + 2] = rects[i].w; out[4 * i + 3] = rects[i].h;
  }
  return (int32_t)rects.size();
}

// What jxlhip_encode_animation_rects says of these options before it looks at anything else: 1 and the words in err where it refuses
// them, 0 where it does not.
extern "C" JXLFILETYPEIO_API int32_t jxlhip_selftest_animation_rect_options(int32_t max_rects, int32_t merge_pixels, ErrorInfo* err) {
  const char* why = AnimRectOptionsRefusal(max_rects, merge_pixels);
  if (why) SetEncErr(err, why);
  return why ? 1 : 0;
}

// What jxlhip_encode_animation_changes says of this tolerance: 1 and the words in err where it refuses it, 0 where it does not.
extern "C" JXLFILETYPEIO_API int32_t jxlhip_selftest_animation_tolerance(float tolerance, ErrorInfo* err) {
  const char* why = AnimToleranceRefusal(tolerance);
  if (why) SetEncErr(err, why);
  return why ? 1 : 0;
}

// AnimSampleChanged (enc_animation.h) on n pairs of samples, their bits in the low bytes of a[i] and b[i].  kind: 0 u8, 1 u16, 2
// binary16, 3 binary32.  out[i]: 1 changed, 0 unchanged.
extern "C" JXLFILETYPEIO_API void jxlhip_selftest_animation_sample_changed(int32_t kind, const uint32_t* a, const uint32_t* b, size_t n, float tolerance,
                                                                           uint8_t* out) {
  for (size_t i = 0; i < n; i++) out[i] = AnimSampleChanged((AnimSample)kind, a[i], b[i], tolerance) ? 1 : 0;
}
