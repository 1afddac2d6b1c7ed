// ORACLE — test infrastructure only (see jxo_common.h header).
// Public C++ surface of the CPU restatement: whole-file decode and encode.
#pragma once
#include "jxo_common.h"
#include "jxo_headers.h"
#include "jxo_vardct.h"
#include <functional>

namespace jxo {

// Intermediate results kept for per-stage parity tests against the HIP path.
// Plane layouts are the ones documented in DESIGN.md ("Data layout in HBM").
struct StageDump {
  int w8 = 0, h8 = 0;                      // frame size in 8x8 blocks
  int wp = 0, hp = 0;                      // frame size padded to blocks (8*w8, 8*h8)
  std::vector<int32_t> lf_quant[3];        // X,Y,B quantised LF, w8*h8
  std::vector<float> lf[3];                // dequantised (+CfL, +smoothing) LF, w8*h8
  std::vector<uint8_t> strategy;           // per 8x8 cell: strategy id | 0x80 if first (top-left) cell
  std::vector<int32_t> raw_quant;          // per cell
  std::vector<uint8_t> sharpness;          // per cell
  std::vector<int8_t> ytox, ytob;          // per 64x64 tile, ceil(w8/8) x ceil(h8/8)
  std::vector<int32_t> qcoef[3];           // quantised HF coefficients, footprint layout, wp*hp
  std::vector<float> xyb_idct[3];          // after IDCT, wp*hp (cropped to frame size: w*h)
  std::vector<float> xyb_filtered[3];      // after Gaborish + EPF, w*h
  std::vector<int32_t> alpha;              // decoded alpha (w*h) if present
  // Modular frames: the frame-level channel list as coded (before the inverse transforms), zero-size channels included
  std::vector<std::vector<int32_t>> mod_coded;
  std::vector<int32_t> mod_coded_w, mod_coded_h;
};

struct DecodeResult {
  ImageMetadata meta;
  FrameHeader frame;
  ContainerInfo boxes;
  int num_channels = 0;         // 1,2,3,4 (gray[+a], rgb[+a])
  int out_w = 0, out_h = 0;     // size of `pixels`: the frame size with the header's orientation applied (5..8 swap the sides)
  int bits_out = 8;             // 8: `pixels` holds u8 samples; 16: little-endian u16 samples (streams of more than 8 bits per sample)
  bool out_float = false;       // float-sample streams: bits_out 16 = binary16, 32 = binary32 (little-endian bit patterns)
  std::vector<uint8_t> pixels;  // interleaved, tight rows; CMYK (black extra channel): C, M, Y, K [, A] with 0 = no ink (the
                                // reference inverts the stored samples for its host, Decoder/JxlDecoder.cpp:159-215)
  std::vector<uint8_t> icc;     // embedded ICC profile (what the reference hands to setIccProfile for original-profile streams)
  bool cmyk = false;
  StageDump dump;
};

struct DecodeOptions {
  bool want_dump = false;
  int num_threads = 1;
};

void DecodeJxl(const uint8_t* data, size_t size, const DecodeOptions& opt, DecodeResult& out);

// Side information of a lossy frame that the writer can vary (parity-test coverage; the defaults are what every stream carried
// before this existed and keep its bytes).  Every float that the stream stores as F16 is rounded first and the writer itself works
// with the rounded value.  The layout is mirrored by tests/oracle_lib.py (SideInfo) and handed over through jxo_set_next_side_info.
//
// The formula modes draw from one integer hash of (seed, x, y, k), all arithmetic modulo 2^32:
//   u = seed * 0x9E3779B1 + x * 0x85EBCA6B + y * 0xC2B2AE35 + k * 0x27D4EB2F;  u ^= u >> 15;  u *= 0x2C1B3C6D;  u ^= u >> 12
//   ytox[ty, tx] = (u(seed, tx, ty, 0) & 255) - 128, ytob[ty, tx] = (u(seed, tx, ty, 1) & 255) - 128   (64 x 64 tiles of the frame)
//   sharpness[by, bx] = u(seed, bx, by, 2) & 7                                                          (8 x 8 cells of the frame)
// and then pin the extremes: tile 0 of the frame holds (ytox, ytob) = (-128, 127), tile 1 (127, -128); cell 0 holds 0, cell 1 holds 7.
struct SideInfo {
  int32_t cfl_mode = 0;        // 0: both maps zero (Zero-predictor leaf, every residual 0); 1: fitted - per tile the least-squares factor of X
                               // and of B on the dequantised Y over the tile's HF coefficients (Zero predictor); 2: formula (Gradient predictor)
  int32_t sharp_mode = 0;      // 0: 4 in every cell (Zero predictor + leaf offset 4, every residual 0); 1: formula (Gradient predictor);
                               // 2: `sharp_value` in every cell (Zero predictor, no leaf offset: one real token per cell)
  int32_t sharp_value = 4;
  uint32_t seed = 0;
  int32_t refuse = 0;          // REFUSAL TESTS ONLY.  1: the last cell's sharpness is 8; 2: the last tile's ytox is 128 (outside int8)
  int32_t custom_cfl = 0;      // LfGlobal carries the five chroma-from-luma parameters below
  uint32_t color_factor = 84;
  float base_x = 0.f, base_b = 1.f;
  int32_t ytox_lf = 0, ytob_lf = 0;          // -128 ... 127
  int32_t custom_lf_factors = 0;
  float lf_factor[3] = {1.0f / 32, 1.0f / 4, 1.0f / 2};   // as stored: 128 x the step of X, Y, B at global_scale * quant_lf = 65536
  int32_t x_qm_scale = -1, b_qm_scale = -1;  // -1: the defaults 3 and 2
  int32_t custom_gab = 0;
  float gab_w1[3] = {0, 0, 0}, gab_w2[3] = {0, 0, 0};
  int32_t custom_sharp_lut = 0;
  float sharp_lut[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int32_t custom_epf_weights = 0;
  float epf_channel_scale[3] = {40.0f, 5.0f, 3.5f};
  int32_t custom_epf_sigma = 0;
  float epf_quant_mul = 0.46f, epf_pass0_sigma_scale = 0.9f, epf_pass2_sigma_scale = 6.5f, epf_border_sad_mul = 2.0f / 3;
  int32_t custom_transform = 0;   // custom transform data: inverse opsin matrix and biases at their defaults as F16 rounds them, and these
  float quant_bias[4] = {0, 0, 0, 0};   // quant biases (the writer dequantises Y with them for its chroma-from-luma compensation)
};
uint32_t SideInfoHash(uint32_t seed, uint32_t x, uint32_t y, uint32_t k);

struct EncodeParams {
  SideInfo side;
  // Explicit MA trees (parity-test coverage; empty: the writer's own).  7 ints per node - property (or -1 for a leaf), split value, child taken when
  // property > split value, the other child, predictor, offset, multiplier - linked by index, node 0 the root, children after their parent.
  // [0]: the whole tree of a lossless frame; [1]: what a lossy frame's alpha channel is coded with (in place of both alpha leaves of the
  // frame's tree); [2]: what each of the three LF channels is coded with (in place of their leaves, below the tree's channel splits)
  std::vector<int32_t> tree[3];
  // Explicit transform list of a lossless frame (parity-test coverage; have_transforms false: the writer's own choice).  Applied forward in
  // order and written to the GlobalModular header in that order.  Flat ints, one entry after the other:
  //   0, begin_c, rct_type                                   an RCT
  //   1, begin_c, num_c                                      a Palette (channel indices as MetaApplyTransforms counts them)
  //   2, n, n x (horizontal, in_place, begin_c, num_c)       a Squeeze; n = 0: the default parameters, written as a count of 0
  //   3, id, then the header fields of that transform id     REFUSAL TESTS ONLY, last entry only: written as given, nothing is done to
  //      (0: begin_c, rct_type; 1: begin_c, num_c, nb_colors, nb_deltas, predictor; 2: n, n x 4)   the channels and nothing is checked
  bool have_transforms = false;
  std::vector<int32_t> transforms;
  float distance = 1.0f;
  bool lossless = false;
  int effort = 7;
  // 0: activity heuristic (default), 1: DCT8 only, 2: seeded pseudo-random mix of every supported
  // strategy (parity-test coverage), 3: every block of one strategy (`fixed_strategy`) where it fits
  int strategy_mode = 0;
  int fixed_strategy = 0;
  uint32_t seed = 1;
  int epf_iters = -1;     // -1: by distance
  bool gaborish = true;
  bool container = true;
  bool adaptive_lf_smoothing = true;
  int lossless_predictor = 6;   // leaf predictor for lossless modular (6 = weighted)
  bool lossless_squeeze = false;
  int lossless_tree = 0;        // 0: contexts from the weighted predictor's error (property 15); 1: local-gradient contexts (W-NW, NW-N)
  int num_threads = 1;
  int orientation = 1;          // EXIF orientation written to the header (1..8); the pixels handed in are the STORED image
  int bits = 8;                 // bits per sample signalled in the header (8..16); above 8 the input samples are uint16
  // colour encoding signalled in the header; the pixels handed in are ALREADY in that space (lossy frames are converted to XYB from
  // it).  0: sRGB; 1: Display P3 (sRGB transfer); 2: BT.709 transfer, sRGB primaries; 3: BT.2100 primaries, linear;
  // 4: BT.2100 primaries, PQ (intensity target 10000); 5: linear sRGB; 6: HLG written to the header only (refusal tests);
  // 7: Adobe RGB (custom primaries + gamma); 8: DCI-P3 (DCI white, gamma 2.6); 9: sRGB primaries, D50 white, linear
  int colour = 0;
  int float_samples = 0;        // 0: integer samples; 16 / 32: binary16 / binary32 samples (input arrays of that float type)
  std::vector<uint8_t> icc;     // embedded ICC profile instead of the enumerated colour encoding
  int num_passes = 1;                 // lossy: 2 or 3 = progressive passes (coefficient bits split by the shifts 1 / 2, 1)
  bool palette = false;               // lossless: colour (+ alpha) channels through a Palette transform when the image has at most 1024 colours
  bool lf_contexts = false;           // lossy: a block-context map with LF thresholds (quartiles of the quantised LF) and two quant-field thresholds
  bool custom_orders = false;         // lossy: coefficient orders sorted by how often each position is non-zero (per order bucket and channel)
  bool custom_quant_tables = false;   // lossy: every dequantisation table written explicitly (parameters scaled per table by `seed`)
  int animation_frames = 1;     // > 1: an animation; frame k > 0 shows the picture rotated by 180 degrees / inverted (any decoder
                                // that returns something other than the first frame is caught)
  bool mislabel_afv = false;    // lossy, REFUSAL TESTS ONLY: some 8x8 DCT blocks are written to the block-metadata stream as AFV0..AFV3 (the
                                // coefficients stay those of the 8x8 DCT, so the stream is not a meaningful picture): a decoder without AFV must refuse it
  bool premultiplied_alpha = false;   // the alpha channel is signalled as associated; the colour samples handed in are ALREADY premultiplied
  // lossy: the varblock layout in place of the writer's heuristics (parity-test coverage).  4 ints per block - strategy, bx, by (origin
  // cell), raw quant (1..256; 0: the writer's own) - anywhere the format allows, aligned to the block's size or not: disjoint, inside
  // the frame and inside their 32x32-cell group (checked).  Every cell left over becomes DCT8.
  bool have_varblocks = false;
  std::vector<int32_t> varblocks;
  // lossy, one-LF-group frames, REFUSAL TESTS: the strategy and quant rows of the block-metadata channel written exactly as given
  // (2 ints per block: strategy, raw quant), count = their number.  The rest of the frame is that of the longest prefix the placement
  // rule accepts, completed with DCT8; a decoder refuses an invalid sequence before it reads the HF sections.
  std::vector<int32_t> varblock_sequence;
  bool cmyk = false;            // lossless only: nch 4 / 5 = C, M, Y, K [, A] as STORED (0 = full ink); K goes to a black extra channel
};

// rgba: interleaved RGBA8 (or RGB8 / Gray8 / GrayA8 according to nch), tight rows.
// Token counts of the last VarDCT frame this thread encoded: LF coefficients, HF metadata, HF coefficients, alpha.
void SetLastEncodeTokenCounts(const uint64_t n[4]);
void GetLastEncodeTokenCounts(uint64_t n[4]);
std::vector<uint8_t> EncodeJxl(const uint8_t* px, uint32_t w, uint32_t h, int nch, const EncodeParams& p,
                               const uint8_t* exif = nullptr, size_t exif_size = 0, const uint8_t* xmp = nullptr,
                               size_t xmp_size = 0);

void ParallelFor(int n, int num_threads, const std::function<void(int)>& fn);

}  // namespace jxo
