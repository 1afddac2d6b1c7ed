// Device-side description of one image being encoded (encode_kernels.hip / encoder.cc).
#pragma once
#include <stdint.h>
#include "dev_types.h"

namespace jxlhip {

struct DevToken { uint32_t ctx, value; };   // after the reverse ANS pass `ctx` holds flushed << 16 | flush bits

// leaf (= context) ids of the encoder's fixed MA tree, in decode order (encoder.cc: MakeEncoderTree)
enum EncLeaf : uint32_t {
  kLeafAlpha = 0, kLeafSharp = 1, kLeafAlphaGlobal = 2, kLeafCfl = 3, kLeafLfB = 4, kLeafQf = 5, kLeafStrategy = 6, kLeafLfX = 7,
  kLeafLfY = 8, kNumEncLeaves = 9
};
constexpr uint32_t kEncSyms = 128;            // token alphabet of the fixed hybrid-uint config (4, 2, 0)
constexpr uint32_t kAcContexts = 495 * 15;    // one preset, default block-context map
constexpr uint32_t kLfTokCap = 3 * 65536;     // tokens per LF group: LF coefficients
constexpr uint32_t kMetaTokCap = 2 * 65536;   // ... and the two rows of the block info (strategies, quant field)
constexpr uint32_t kCflTokCap = 2 * 1024;     // ... and, with fitted chroma-from-luma maps, the two maps of its up to 32 x 32 tiles
constexpr uint32_t kMetaCflBit = 0x80000000u; // n_meta: set when the stream begins with the tokens of the two maps
constexpr uint32_t kAcTokCap = 3 * 65 * 1024; // tokens per group: 1 + 64 per (block, channel)
constexpr int32_t kMaxQuantHf = 32767;        // largest |quantised HF value| written: hf_decode_kernel keeps each value as an int16
// Capacities and the sample depth (jxlhip_save_pixels takes up to 16-bit integers and binary16 / binary32 samples).  The token COUNTS
// do not depend on the depth: one token per sample, a group is at most 256 x 256 samples per channel.  What grows with the depth is
// the value a token carries, and with it the bits a token takes in its section:
//   - a sample of a lossless frame is below 2^16; YCoCg-R puts the chroma into [-65535, 65535] (an int32 plane holds it with room to
//     spare), a gradient residual of such planes is below 2^17 in magnitude, PackSigned of it below 2^18: token at most
//     16 + 13 * 4 + 3 = 71, 15 raw bits;
//   - the alpha of a lossy binary32 frame is the sample's bit pattern (an int32): a residual packs into any 32-bit value, token at most
//     16 + 27 * 4 + 3 = 127 < kEncSyms, 29 raw bits.
// A token writes at most one 16-bit flush of the rANS state and its raw bits: 16 + 29 = 45 bits for a 32-bit value, so the 6 bytes
// (48 bits) per token that every section buffer (sec_cap) allows hold the worst cases - a 256 x 256 group of 16-bit RGBA noise
// (4 x 65536 tokens of at most 16 + 15 bits) and one of binary32 alpha bit patterns (65536 tokens of at most 45 bits) - with the 32
// bits of the final state and the group header inside the 256 bytes of slack.  WaveWriter::PutParallel takes up to 48 bits per lane.
constexpr uint32_t kAlphaTokCap = 65536;      // one alpha sample per pixel of a 256 x 256 group, whatever its depth
constexpr uint32_t kLlTokCap = 4 * 65536;     // lossless: up to four channels per group, whatever their depth
constexpr uint32_t kSecBytesPerTok = 6;       // bytes of section buffer per token (see above: 45 bits at most)

enum EncSampleType : int32_t { kSampleUint8 = 0, kSampleUint16 = 1, kSampleFloat16 = 2, kSampleFloat32 = 3 };   // ImageChannelRepresentation
enum EncTransfer : int32_t { kTransferLinear = 0, kTransferSrgb = 1, kTransfer709 = 2, kTransferPq = 3 };

struct EncCodeDev {
  const uint8_t* ctx_map;
  const uint16_t* freq;    // [cluster * kEncSyms + symbol]
  const uint16_t* start;
  const uint16_t* rmap;    // [cluster * 4096 + start + offset]
  uint32_t num_clusters, num_ctx;
};

struct EncImage {
  int32_t w, h, w8, h8, wp, hp;
  int32_t xg, yg, ng, xlf, ylf, nlf;
  int32_t gray, has_alpha, gab, lossless;
  // source: the BGRA8 surface of SaveImage (host layout BitmapData, `stride` bytes per row; 8-bit input of jxlhip_save_pixels is
  // repacked into one), or `src_nch` interleaved samples per pixel in tight rows (`stride` = w * src_nch * sample bytes)
  const uint8_t* bgra;
  int64_t stride;
  int32_t src_type;         // EncSampleType of the interleaved samples
  int32_t src_nch;          // interleaved samples per pixel: Gray | Gray,A | R,G,B | R,G,B,A (0: the BGRA8 surface)
  int32_t transfer;         // transfer function of the samples: 0 linear, 1 sRGB, 2 BT.709, 3 PQ (EncTransfer)
  float sample_scale;       // integer samples: 1 / (2^bits - 1); floats: unused
  int32_t pad0;
  int32_t use_matrix;       // 1: icc_to_srgb takes the linear samples of the space's primaries to linear sRGB (relative to 255 nits)
  uint32_t* flags;          // [0] some pixel is not gray, [1] some pixel has alpha < 255
  // documents with an (evaluated, matrix / TRC) ICC profile: 3 x 256 samples -> linear of the profile, then 3x3 -> linear sRGB
  const float* icc_lin;     // nullptr: the samples are in the space `transfer` / `use_matrix` describe
  float icc_to_srgb[9];
  // planes
  float* xyb[3];            // w*h
  float* pad[3];            // wp*hp: (inverse-Gaborish sharpened) XYB, edge-replicated to whole 8x8 cells
  int32_t* alpha_px;        // w*h
  int32_t* lfq[3];          // w8*h8 quantised LF (X, Y, B)
  int32_t* rawq;            // w8*h8 raw quant field (1..256)
  // chroma-from-luma maps fitted per 64x64 tile (cfl != 0; null otherwise: factor 0 for X and 1 for B everywhere)
  int8_t* ytox;             // ceil(w8 / 8) * ceil(h8 / 8)
  int8_t* ytob;
  int32_t cfl;              // JxlHipLossyOptions::chroma_from_luma
  uint32_t meta_cap;        // tokens of tok_meta per LF group: kMetaTokCap, + kCflTokCap with fitted maps
  // varblocks: `squares` = 0: 8x8 DCTs only (the fast effort); 1: 8x8 / 16x16 / 32x32; 2: also 64x64 and the rectangular
  // 16x8 ... 64x32 shapes (the default effort)
  int32_t squares, pad1;
  float* act;               // w8*h8 activity of Y per cell (standard deviation)
  uint8_t* strat;           // w8*h8: strategy code of the varblock covering the cell | 0x80 on its first cell
  int32_t* qs[3];           // w8*h8*64 quantised coefficients: scan position k of a varblock at its covered cell (k >> 6, row-major) * 64 + (k & 63)
  uint8_t* nz[3];           // per cell: the non-zero context value of the varblock covering it, (count + covered - 1) >> log2(covered)
  uint16_t* nzc[3];         // per first cell: number of non-zero HF coefficients of the varblock
  uint16_t* last[3];        // per first cell: scan position of the last non-zero coefficient (0: none)
  // quantiser
  float inv_mul_lf[3];      // 1 / (m_lf * inv_global_scale / quant_lf)
  float mul_lf_y;           // LF dequant step of Y (chroma-from-luma of the LF uses the dequantised Y)
  float inv_gs;             // 65536 / global_scale
  float x_dm, b_dm;         // 0.8 ^ (x_qm_scale - 2), 0.8 ^ (b_qm_scale - 2)
  float qbias1, qbias3;     // quantisation bias of |q| == 1 (Y) and the 1/q term
  float gab_w[3][3];
  // per order bucket (13): inverse natural order (stored index -> scan position); per quant table (17): 3 * n dequantisation
  // multipliers in the stored layout; per transform length N = 8, 16, 32, 64 (index 0..3): the basis B[k * N + n] and the same divided
  // by N; per c = 1, 2, 4, 8: the c x c basis (LF values of a varblock from its lowest coefficients) and the resample scales
  const uint16_t* scan_of[13];
  const float* dq[17];
  const float* basis[4];
  const float* basis_div[4];
  const float* bsmall[4];
  const float* rs;          // [(lcy * 4 + lcx) * 64 + ky * 8 + kx]: scale of coefficient (ky, kx) of the lowest cy x cx
  // tokens
  DevToken* tok_lf;         // [nlf][kLfTokCap]
  DevToken* tok_meta;       // [nlf][meta_cap]
  DevToken* tok_ac;         // [ng][kAcTokCap]
  DevToken* tok_alpha;      // [ng][kAlphaTokCap]
  uint32_t* n_ac;           // [ng]
  uint32_t* n_meta;         // [nlf] tokens of the block-info stream (| kMetaCflBit)
  uint32_t* hist_mod;       // [kNumEncLeaves][kEncSyms]
  uint32_t* hist_ac;        // [kAcContexts][kEncSyms]
  // lossless (Modular) frames: whole-image integer channels, tokens per group
  int32_t* ll_plane[4];
  int32_t ll_nch, ll_rct;   // ll_rct: RGB is coded as YCoCg-R (reversible colour transform 6)
  DevToken* tok_ll;         // [ng][4 * 65536]
  uint32_t ll_tok_extra, pad2;   // tokens ahead of the samples in group 0's stream (a palette's colours in a one-group frame)
  // entropy coding
  EncCodeDev mcode, acode;
  uint8_t* sec_bytes;       // section s at s * sec_cap
  uint32_t* stream_state;   // final rANS state per token stream (lossy frames: 2 per LF group, 2 per group, 1 global alpha)
  uint64_t* sec_bits;       // bits written per section
  uint64_t sec_cap;
};

// Which images a batch kernel covers and where each one's share of the grid begins (encode_kernels.hip, "batch forms"): entry k is a
// run of workgroups (the compaction: sections) of image image_of[k] of the batch's record array, beginning at that image's workgroup
// wg0[k]; first[k] counts the workgroups of the entries before it.  An image may have several entries: the reverse pass of the Modular
// streams lists the workgroups with the LF streams of every image first, so that the longest recurrences of the batch all start at once.
struct EncBatchTable {
  const uint32_t* first;      // [entries], ascending, first[0] = 0
  const int32_t* image_of;    // [entries]
  const uint32_t* wg0;        // [entries]
  int32_t entries, pad;
};

// The searched lossless stream of efforts 8 and 9 (lossless_kernels.hip; the rules: DESIGN.md §2, "Lossless efforts 8 and 9").
constexpr uint32_t kPalCap = 1024;        // most colours a palette is written for
constexpr uint32_t kPalSlots = 4096;      // slots of the colour hash set (a power of two, four times the cap)
constexpr int kLlSlots = 10;              // candidate planes costed in one pass: R, G, G-R, G-((R+B)>>1), B, B-R, Y, Co, Cg, alpha
constexpr int kLlPreds = 5;               // predictors 1..5: West, North, average, Select, gradient
constexpr int kWpLeaves = 11;             // buckets of property 15 (kWpCuts of lossless_kernels.hip)
constexpr uint32_t kLlMaxLeaves = 4 * kWpLeaves + 4;

struct LlSearch {
  // palette: the set of distinct pixels over the coded channels, slot = 0 (empty) or 1 << 32 | key; key = channel k in byte k
  unsigned long long* pal_set;   // [kPalSlots]
  uint32_t* pal_count;           // [0] colours inserted, [1] set once more than kPalCap were seen (or the set ran full)
  const uint16_t* pal_index;     // [kPalSlots]: slot -> index in the sorted palette
  // search: token histograms of the residuals of every (candidate plane, predictor)
  uint32_t* hist_search;         // [kLlSlots * kLlPreds][kEncSyms]
  int32_t from_planes;           // 0: candidates from the BGRA surface (RGB); 1: the ll_nch planes as they are (gray, palette indices)
  // what was chosen
  int32_t rct_type;              // 0..6 of permutation 0 (RGB), 0 otherwise
  int32_t pred[4];               // predictor of coded channel c (1..6)
  int32_t wp_ctx;                // 1: the context of a sample follows property 15
  uint8_t ctx[4][kWpLeaves + 1]; // context (leaf id) of channel c and bucket k of property 15 (every bucket the same without wp_ctx)
  // forward weighted predictor: prediction and property 15 of every sample, histogram of its residuals per channel
  int32_t* wp_pred[4];
  int32_t* wp_prop[4];
  uint32_t* hist_wp;             // [4][kEncSyms]
  uint32_t* hist_ll;             // [kLlMaxLeaves][kEncSyms]
};

// Distance map of a reconstruction against its original, both as XYB planes (distance_kernels.hip; the rules and the constants:
// DESIGN.md §2, "Distance map: rules of this project")
struct DistMap {
  int32_t w, h, w8, h8;
  const float* orig[3];     // w*h, tight rows
  const float* recon[3];    // rows `recon_stride` floats apart
  int32_t recon_stride, pad0;
  float* mask;              // w*h: M of the original
  float* cell;              // w8*h8: T per 8x8 cell
  float a0, k;              // masking constant, calibration
  float s2[3];              // squared channel weights
};

}  // namespace jxlhip
