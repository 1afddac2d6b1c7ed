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
#include "dev_util.h"
#include "enc_types.h"
#include "host_parse.h"
#include "host_write.h"
#include "icc.h"

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
