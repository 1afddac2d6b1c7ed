/*
 * C-ABI of libJpegXLFileTypeIO (MI355X-native) — the drop-in boundary.
 *
 * Part 1 replaces, symbol for symbol, the three exports of the reference's native IO DLL:
 *   reference: src/JxlFileTypeIO/JxlFileTypeIO.h:29-43 (exports)
 *              src/JxlFileTypeIO/Common.h:17-60 (BitmapData, ImageChannelRepresentation, ProgressProc, IOCallbacks, ErrorInfo)
 *              src/JxlFileTypeIO/Decoder/JxlDecoderTypes.h:17-71 (DecoderStatus, DecoderImageFormat, KnownColorProfile, DecoderCallbacks)
 *              src/JxlFileTypeIO/Encoder/JxlEncoderTypes.h:17-42 (EncoderStatus, EncoderOptions, EncoderImageMetadata)
 *   bound by:  src/Interop/JpegXL_X64.cs:19-39 (LibraryImport "JpegXLFileTypeIO_X64.dll", stdcall)
 * `__stdcall` is a no-op on x64/ARM64 and is defined empty here.  Struct layouts are identical under LP64 and LLP64
 * (checked by the static asserts at the end).  `bool` is one byte (src/Interop/DecoderCallbacks.cs:22-34).
 *
 * Part 2 (jxlhip_*) is the device-resident batch entry point used by bench.py / tests: same decode path,
 * but bitstreams and RGBA8 outputs stay in HBM and several images are decoded per call.
 *
 * Part 3 (jxlhip_save_pixels) is SaveImage for every sample type LoadImage hands out: 8- to 16-bit integers, binary16 and binary32,
 * Gray | GrayA | RGB | RGBA, in any of the colour encodings the host knows by name.
 *
 * Part 4 (jxlhip_encode_batch) encodes many device-resident images in one call.
 *
 * Part 5 (jxlhip_animation_*) decodes every displayed image of an animated file into device memory, in file order.
 *
 * Part 6 (jxlhip_encode_animation, jxlhip_encode_animation_rects, jxlhip_encode_animation_changes) encodes a stack of device-resident frames as one animated file: each
 * frame as what changed, in one rectangle or in several.
 */
#ifndef JXLFILETYPEIO_H_
#define JXLFILETYPEIO_H_

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifndef JXL_STDCALL
#define JXL_STDCALL
#endif
#if defined(__GNUC__)
#define JXLFILETYPEIO_API __attribute__((visibility("default")))
#else
#define JXLFILETYPEIO_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Common.h:17-23 */
typedef struct BitmapData {
  uint8_t* scan0; /* BGRA8, `stride` bytes per row, host-owned, read-only */
  uint32_t width;
  uint32_t height;
  uint32_t stride;
} BitmapData;

/* ---- Common.h:33-39 */
typedef int32_t ImageChannelRepresentation;
enum { ImageChannelRepresentation_Uint8 = 0, ImageChannelRepresentation_Uint16, ImageChannelRepresentation_Float16, ImageChannelRepresentation_Float32 };

/* ---- Common.h:41-53 */
typedef bool(JXL_STDCALL* ProgressProc)(int32_t progressPercentage);
typedef int32_t(JXL_STDCALL* WriteCallback)(const uint8_t* buffer, size_t sizeInBytes); /* returns HRESULT */
typedef int32_t(JXL_STDCALL* SeekCallback)(uint64_t position);                          /* absolute; returns HRESULT */
typedef struct IOCallbacks {
  WriteCallback Write;
  SeekCallback Seek;
} IOCallbacks;

/* ---- Common.h:55-60 */
typedef struct ErrorInfo {
  char errorMessage[256]; /* NUL-terminated, written only when the message fits 255 chars (Common.cpp:18-53) */
} ErrorInfo;

/* ---- JxlDecoderTypes.h:17-32 */
typedef int32_t DecoderStatus;
enum {
  DecoderStatus_Ok = 0, DecoderStatus_NullParameter, DecoderStatus_InvalidParameter, DecoderStatus_OutOfMemory,
  DecoderStatus_HasAnimation, DecoderStatus_HasMultipleFrames, DecoderStatus_ImageDimensionExceedsInt32,
  DecoderStatus_UnsupportedChannelFormat, DecoderStatus_CreateLayerError, DecoderStatus_CreateMetadataError,
  DecoderStatus_DecodeError, DecoderStatus_MetadataError, DecoderStatus_InvalidFileSignature
};
/* ---- JxlDecoderTypes.h:34-39 */
typedef int32_t DecoderImageFormat;
enum { DecoderImageFormat_Gray = 0, DecoderImageFormat_Rgb, DecoderImageFormat_Cmyk };
/* ---- JxlDecoderTypes.h:41-51 */
typedef int32_t KnownColorProfile;
enum {
  KnownColorProfile_Srgb = 0, KnownColorProfile_LinearSrgb, KnownColorProfile_LinearGray, KnownColorProfile_GraySrgbTRC,
  KnownColorProfile_DisplayP3, KnownColorProfile_Rec709, KnownColorProfile_Rec2020Linear, KnownColorProfile_Rec2020PQ
};
/* ---- JxlDecoderTypes.h:53-71 */
typedef void(JXL_STDCALL* DecoderSetBasicInfo)(int32_t width, int32_t height, DecoderImageFormat format,
                                               ImageChannelRepresentation channelFormat, bool hasTransparency);
typedef bool(JXL_STDCALL* DecoderSetMetadata)(uint8_t* data, size_t length);
typedef bool(JXL_STDCALL* DecoderSetKnownColorProfile)(KnownColorProfile profile);
typedef bool(JXL_STDCALL* DecoderSetLayerData)(uint8_t* pixels, char* name, size_t nameLength);
typedef struct DecoderCallbacks {
  DecoderSetBasicInfo setBasicInfo;
  DecoderSetMetadata setIccProfile;
  DecoderSetKnownColorProfile setKnownColorProfile;
  DecoderSetMetadata setExif;
  DecoderSetMetadata setXmp;
  DecoderSetLayerData setLayerData;
} DecoderCallbacks;

/* ---- JxlEncoderTypes.h:17-25 */
typedef int32_t EncoderStatus;
enum { EncoderStatus_Ok = 0, EncoderStatus_NullParameter, EncoderStatus_OutOfMemory, EncoderStatus_UserCanceled,
       EncoderStatus_EncodeError, EncoderStatus_WriteError };
/* ---- JxlEncoderTypes.h:27-32 */
typedef struct EncoderOptions {
  float distance;
  int32_t effort;
  bool lossless;
} EncoderOptions;
/* ---- JxlEncoderTypes.h:34-42 */
typedef struct EncoderImageMetadata {
  uint8_t* exif; /* already carries the 4-byte big-endian TIFF offset prefix (src/Exif/ExifWriter.cs:86-90) */
  size_t exifSize;
  uint8_t* iccProfile;
  size_t iccProfileSize;
  uint8_t* xmp;
  size_t xmpSize;
} EncoderImageMetadata;

/* ---- JxlFileTypeIO.h:29 — (major<<24)|(minor<<16)|(patch<<8), unpacked by src/Interop/JpegXLNative.cs:40-42 */
JXLFILETYPEIO_API uint32_t JXL_STDCALL GetLibJxlVersion(void);

/* ---- JxlFileTypeIO.h:31-35 -> Decoder/JxlDecoder.cpp:796-852.
 * Callback order: setBasicInfo, then colour profile / Exif / XMP, then setLayerData exactly once.
 * Pixels handed to setLayerData: interleaved, tight rows, Gray|GrayA|RGB|RGBA, 8 bits per sample. */
JXLFILETYPEIO_API DecoderStatus JXL_STDCALL LoadImage(DecoderCallbacks* callbacks, const uint8_t* data, size_t dataSize,
                                                      ErrorInfo* errorInfo);

/* ---- JxlFileTypeIO.h:37-43 -> Encoder/JxlEncoder.cpp:147-392 */
JXLFILETYPEIO_API EncoderStatus JXL_STDCALL SaveImage(const BitmapData* bitmap, const EncoderOptions* options,
                                                      const EncoderImageMetadata* metadata, IOCallbacks* callbacks,
                                                      ErrorInfo* errorInfo, ProgressProc progressCallback);

/* =====================================================================================================
 * Part 2: device-resident batch decode (not in the reference; used by bench.py and the GPU parity tests).
 * ===================================================================================================== */
typedef struct JxlHipDecoder JxlHipDecoder;

typedef struct JxlHipImageInfo {
  int32_t width, height;
  int32_t num_channels;   /* 1..4, interleaved u8 */
  int32_t has_alpha;
  int32_t xsize_blocks, ysize_blocks;
  int32_t num_groups, num_lf_groups;
  int32_t epf_iters, gaborish;
  uint64_t codestream_bytes;
  int32_t bytes_per_sample;   /* 1: u8 output; 2: u16 (more than 8 bits per sample) or binary16; 4: binary32 */
  int32_t reserved;           /* 1: the samples are floats (binary16 / binary32) */
} JxlHipImageInfo;

/* device < 0: current HIP device.  Returns NULL on failure (message in err, may be NULL). */
JXLFILETYPEIO_API JxlHipDecoder* jxlhip_decoder_create(int32_t device, ErrorInfo* err);
JXLFILETYPEIO_API void jxlhip_decoder_destroy(JxlHipDecoder* dec);

/* Parses headers only (host). */
JXLFILETYPEIO_API DecoderStatus jxlhip_peek(const uint8_t* data, size_t size, JxlHipImageInfo* info, ErrorInfo* err);

/* Decodes n files.  host_data[i]/sizes[i]: the file bytes in host memory (headers are parsed on the host).
 * dev_data[i]: the same bytes already resident in HBM, or NULL (then they are uploaded inside the call).
 * dev_out[i]: device buffer of width*height*num_channels*bytes_per_sample bytes receiving interleaved u8 (or u16) pixels.
 * With the option "downscale" = 8 the image is written at ceil(width/8) x ceil(height/8) pixels instead (width, height as
 * jxlhip_peek reports them, i.e. as displayed), tight rows, same channels / sample type / colour encoding / orientation: the
 * buffer must hold ceil(width/8)*ceil(height/8)*num_channels*bytes_per_sample bytes and nothing behind them is written.
 * The call returns after enqueueing unless `synchronize` is non-zero.  What `stream` (a hipStream_t, may be NULL = a stream of the
 * decoder's own) orders, and what it does not:
 *  - OUTPUTS are ordered on `stream`: every write to dev_out[i] is enqueued there or joined to it by an event, so work enqueued on
 *    `stream` after the call sees the finished pixels, and the buffers may still be in use by work enqueued on `stream` before it.
 *  - INPUT is not: the entropy stages run on streams of the decoder's own, and the LF pre-pass of a frame that fits one group runs
 *    inside the call; both read dev_data[i] without waiting for `stream`.  Resident input must be COMPLETE when the call is made
 *    (synchronise whatever produced it first), and stay untouched until the batch has finished.  host_data is read inside the call.
 *  - Up to three batches are in flight on workspaces of their own; the call blocks the host while the batch three calls back has not
 *    finished.  Options (jxlhip_set_option) are read at the call and hold for that batch.
 * Per-file status is written to statuses[i] on return: final when synchronizing; otherwise only what the host found (parse errors,
 * refusals, the LF pre-pass of one-group frames) - what the device finds is reported by jxlhip_finish(). */
JXLFILETYPEIO_API DecoderStatus jxlhip_decode_batch(JxlHipDecoder* dec, int32_t n, const uint8_t* const* host_data,
                                                    const size_t* sizes, const uint8_t* const* dev_data, uint8_t* const* dev_out,
                                                    void* stream, int32_t synchronize, DecoderStatus* statuses, ErrorInfo* err);
/* Waits for every batch in flight, oldest first, and collects device-side error flags.  statuses (may be NULL): one entry per file
 * of the MOST RECENT batch.  Returns that batch's first status that is not Ok, with its message in err.  When that batch is Ok but
 * an older asynchronous batch failed that nobody has been told of, returns the older batch's status and "an earlier asynchronous
 * batch failed: " followed by the same text that batch would have reported (the image number counts within its own batch); this
 * is reported once.  With nothing in flight, or no batch ever decoded, the call returns at once. */
JXLFILETYPEIO_API DecoderStatus jxlhip_finish(JxlHipDecoder* dec, DecoderStatus* statuses, ErrorInfo* err);

/* Stage taps of the most recent (synchronised) batch, image `index`, for parity tests.  `name` as in
 * DESIGN.md ("lf", "qcoef", "xyb_idct", "xyb_filtered", "strategy", "raw_quant", "sharpness", "alpha", ...).
 * Frames with synthetic noise, under "debug_taps": "noise_rnd" (the random planes R_k, channel 0..2) and "noise" (the convolved
 * planes N_k that the output phase adds), each w * h f32 in tight rows.
 * Copies up to `capacity` bytes device->host; returns the full byte size of the plane (0 = unknown name).
 * `index` counts the batch's decoded images: a layered file contributes one per frame (in file order, in its place among the files),
 * so in a batch with layered files it is not the file index. */
JXLFILETYPEIO_API size_t jxlhip_read_plane(JxlHipDecoder* dec, int32_t index, const char* name, int32_t channel, void* dst,
                                           size_t capacity);

/* Options: "debug_taps" (0/1: keep qcoef / xyb_idct / xyb_filtered stage copies; slow), "lane_stride" (0 = auto,
 * 64 = one section per wavefront ... 1 = one section per lane), "overlap" (0/1: run the LF stage of the next
 * asynchronous batch on a second stream while the previous batch finishes), "band_first_row" / "band_rows" (>= 0: decode only these
 * 256-pixel group rows of a lossy frame into a band-sized buffer), "no_direct" / "mod_lanes64" (launch shapes of the vector loops for
 * small launches as well; same output), "no_stream_pairs" (every fused Gaborish + EPF frame through the four-pixels-per-lane kernel;
 * same output), "no_lf_pipeline" (every LF channel through the row-per-lane prediction pass instead of the register pipeline; same
 * output), "downscale" (1 = full size, the default; 8 = every image of the next batches is decoded at 1:8: one pixel per 8x8 cell -
 * for lossy (VarDCT) frames the LF image after dequantisation and adaptive smoothing through the colour conversion of the full
 * decode, without Gaborish, EPF or noise, alpha as the mean of the cell; for lossless (Modular) frames the mean of the cell's
 * output samples, integers as (sum + n/2) / n over the n pixels of the cell that exist.  The HF coefficients are not reconstructed,
 * and for a frame without alpha not even read: host parsing is the same at both scales, so the same files are accepted and refused,
 * but a damaged HF section of an opaque frame goes unnoticed at 1:8.  Layered files, files with patches and band decodes are refused
 * per image at 1:8 (DecodeError); 2 and 4 are reserved and refused like any other value.  LoadImage always decodes at full size).
 * Returns 1 if the option exists and the value is valid (0: refused, nothing changed). */
JXLFILETYPEIO_API int32_t jxlhip_set_option(JxlHipDecoder* dec, const char* name, int32_t value);

/* Timing of the last synchronised batch: milliseconds per named stage (HIP events on the decode stream). */
JXLFILETYPEIO_API int32_t jxlhip_stage_times(JxlHipDecoder* dec, const char** names, float* ms, int32_t capacity);

/* Cumulative per-stage time over every batch finished since the last reset (asynchronous batches included). */
JXLFILETYPEIO_API int32_t jxlhip_stage_totals(JxlHipDecoder* dec, const char** names, float* ms, int32_t capacity, int32_t* batches,
                                              int32_t reset);

/* Device time of the stages of the calling thread's last LoadImage / lossy SaveImage (HIP events on the streams the kernels were
 * launched on; measurement only: bench.py's single-image and encode workloads read them next to the wall time of the call).  A save
 * at effort 8 or 9 adds one stage per evaluation of its closed loop ("evaluation k (...)": everything from the quant field to the
 * cell distances, host work included).  A lossless save at effort 8 or 9 reports the stages of its search instead ("lossless: colour
 * count", "... transform and predictor search", "... planes", "... weighted pass", "... tokens", "... sections"; the last two once
 * per candidate stream, host work between the launches included); a lossless save at a lower effort leaves the list as it was. */
JXLFILETYPEIO_API int32_t jxlhip_last_load_stage_times(const char** names, float* ms, int32_t capacity);
JXLFILETYPEIO_API int32_t jxlhip_last_save_stage_times(const char** names, float* ms, int32_t capacity);

/* Distance map ("Distance map: rules of this project"; this project's own measure in XYB, not Butteraugli) of
 * picture b against the original a.  Both are BGRA8 in host memory (`stride` bytes per row, alpha ignored) and go through the
 * encoder's sRGB -> XYB conversion.  Writes ceil(w / 8) * ceil(h / 8) cell distances (rows of 8 x 8 cells, top to bottom);
 * `capacity` counts floats and must hold them all. */
JXLFILETYPEIO_API EncoderStatus jxlhip_distance_map(const uint8_t* a_bgra, uint32_t stride_a, const uint8_t* b_bgra, uint32_t stride_b,
                                                    uint32_t width, uint32_t height, float* cell_dist, size_t capacity, ErrorInfo* err);

/* What the closed quantisation loop of the calling thread's last SaveImage measured (efforts 8 and 9 of a lossy save): the cell
 * distances of the evaluation whose quant field was written (up to `capacity` floats are copied), the number of evaluations (0 after
 * a lossless save or an effort below 8: then the other figures are 0 and 0 is returned), the target tau, and the number of cells over tau
 * at the first evaluation (the field effort 7 writes) and at the one written.  Returns the number of cells.  Any pointer may be NULL. */
JXLFILETYPEIO_API size_t jxlhip_last_save_distances(float* dst, size_t capacity, int32_t* evaluations, float* target,
                                                    int32_t* cells_over_target_first, int32_t* cells_over_target_emitted);

/* What the search of the calling thread's last lossless SaveImage chose ("Lossless efforts 8 and 9").  After a
 * lossy save, or a lossless one at an effort below 8, `tier` is 0 and so is everything else.  Byte counts are those of the bare
 * codestream (no container). */
typedef struct JxlHipLosslessInfo {
  int32_t tier;                 /* 8 or 9: the effort tier that ran; 0: none */
  int32_t palette_colours;      /* entries of the palette that replaced the coded channels; 0: no palette */
  int32_t rct_type;             /* reversible colour transform 0..6 of permutation 0 (0: none, 6: YCoCg-R); -1: not RGB, or a palette */
  int32_t num_channels;         /* coded channels (1 behind a palette) */
  int32_t predictor[4];         /* the format's predictor id per coded channel (1..6; 6: weighted); 0 past num_channels */
  int32_t leaves;               /* leaves of the MA tree = contexts */
  int32_t clusters;             /* distributions they were clustered into */
  int32_t fell_back_to_effort7; /* 1: the searched stream was not smaller, so the bytes of effort 7 were written */
  int32_t reserved;
  uint64_t searched_bytes;      /* the searched stream */
  uint64_t effort7_bytes;       /* the stream of effort 7 */
} JxlHipLosslessInfo;
JXLFILETYPEIO_API void jxlhip_last_save_lossless_info(JxlHipLosslessInfo* out);

/* Host-only (no GPU): the embedded ICC profile as LoadImage would hand it to setIccProfile (reference Decoder/JxlDecoder.cpp:652-682);
 * returns its size (0: none) and copies up to `capacity` bytes. */
JXLFILETYPEIO_API size_t jxlhip_parse_icc(const uint8_t* data, size_t size, uint8_t* dst, size_t capacity, DecoderStatus* status, ErrorInfo* err);

/* =====================================================================================================
 * Part 3: saving 16-bit and float images (not in the reference; SaveImage takes a BGRA8 surface and nothing else).
 * ===================================================================================================== */
typedef struct JxlHipPixels {
  const void* data;            /* host memory (jxlhip_encode_batch: device memory), interleaved, channel order Gray | Gray,A | R,G,B | R,G,B,A (as setLayerData hands pixels out) */
  uint32_t width, height;
  uint64_t stride_bytes;       /* >= width * num_channels * bytes per sample */
  int32_t num_channels;        /* 1..4; 2 and 4 carry (unassociated) alpha */
  ImageChannelRepresentation sample_type;   /* Uint8, Uint16, Float16, Float32 */
  int32_t bits_per_sample;     /* integers: 8 for Uint8; 9..16 for Uint16 (samples use the low bits); floats: 0 */
  KnownColorProfile colour;    /* the space the samples are ALREADY in */
} JxlHipPixels;

/* Encodes `pixels` like SaveImage encodes its surface: the same options and effort tiers, container, Exif / XMP boxes, writes of at
 * most 64 KiB, progress checkpoints and cancellation, HRESULT mapping, and the same jxlhip_last_save_stage_times /
 * jxlhip_last_save_distances / jxlhip_last_save_lossless_info afterwards.  What differs:
 *  - The channels are as stated: nothing is dropped or added by looking at the pixels (GetOutputPixelFormat is the plugin's rule).
 *  - Lossy: integer samples mean v / (2^bits - 1), floats mean themselves (samples outside [0, 1] are kept); they reach XYB through
 *    the inverse transfer function and the primaries of `colour`.  Alpha is lossless: integers by value, floats by bit pattern.
 *  - Lossless: integer samples only, exact.  Uint8 input writes SaveImage's streams, the searched tiers 8 and 9 included; deeper
 *    samples get the fixed stream (YCoCg-R, gradient predictor, one context per channel) at every effort.
 *  - `colour` is signalled by its enum: Srgb and LinearSrgb stand for gray with the sRGB curve and linear gray when there are 1 or 2
 *    channels; the other RGB profiles need 3 or 4 channels, the gray profiles 1 or 2.
 * Refused on the host, before any device work, with EncoderStatus_EncodeError and a message each (null pointers:
 * EncoderStatus_NullParameter): zero size, a stride below a row, channels outside 1..4, bits_per_sample that does not fit
 * sample_type, a profile that does not fit the channels, metadata->iccProfile set, and lossless float samples. */
JXLFILETYPEIO_API EncoderStatus jxlhip_save_pixels(const JxlHipPixels* pixels, const EncoderOptions* options,
                                                   const EncoderImageMetadata* metadata, IOCallbacks* callbacks, ErrorInfo* errorInfo,
                                                   ProgressProc progressCallback);

/* What a lossy save may do beyond EncoderOptions.  All zero: the file jxlhip_save_pixels writes. */
typedef struct JxlHipLossyOptions {
  int32_t chroma_from_luma;    /* 0: the per-tile chroma-from-luma maps are all zero; 1: fitted per 64 x 64 tile on the GPU (a least-squares
                                * factor of the X and of the B coefficients on the dequantised Y; usually fewer bytes and better pixels) */
  int32_t reserved[3];         /* must be zero */
} JxlHipLossyOptions;

/* jxlhip_save_pixels with a JxlHipLossyOptions (jxlhip_save_pixels is this call with all of it zero).  Every effort tier, sample type
 * and channel count is supported.  A lossless save ignores what the struct asks for: its bytes are those without it.  Refused on the
 * host, before any device work, with EncoderStatus_EncodeError and a message: chroma_from_luma outside 0..1, a reserved word that is
 * not zero.  When the fit leaves every map value zero (a flat frame), the file is the one of chroma_from_luma = 0, byte for byte. */
JXLFILETYPEIO_API EncoderStatus jxlhip_save_pixels_lossy(const JxlHipPixels* pixels, const EncoderOptions* options, const JxlHipLossyOptions* lossy,
                                                         const EncoderImageMetadata* metadata, IOCallbacks* callbacks, ErrorInfo* errorInfo,
                                                         ProgressProc progressCallback);

/* =====================================================================================================
 * Part 4: batch encode of device-resident images (not in the reference).
 * ===================================================================================================== */
typedef struct JxlHipEncoder JxlHipEncoder;

/* device < 0: current HIP device.  Returns NULL on failure (message in err, may be NULL).  The encoder owns its streams and one
 * device workspace that grows to the largest batch it has seen and is reused: a call that needs no more than an earlier one
 * allocates nothing. */
JXLFILETYPEIO_API JxlHipEncoder* jxlhip_encoder_create(int32_t device, ErrorInfo* err);
JXLFILETYPEIO_API void jxlhip_encoder_destroy(JxlHipEncoder* enc);

/* Encodes n images in one call.  images[i] is a JxlHipPixels whose `data` is a DEVICE pointer (any alignment a sample allows; it is
 * only read); every other field means what it means for jxlhip_save_pixels.  options[i] is per image.  metadata may be NULL, and so
 * may any metadata[i]; Exif and XMP are host pointers.  The call is synchronous: on return every file lies in host memory owned by the
 * encoder (jxlhip_encoder_result).
 * The file of image i is, byte for byte, what jxlhip_save_pixels hands its Write callback, concatenated, for the same pixels in host
 * memory with options[i] and metadata[i].
 * Scope: lossy, and lossless of integer samples, at efforts 1..7.  Efforts 8 and 9 are refused per image (EncoderStatus_EncodeError,
 * decided on the host), and so is everything jxlhip_save_pixels refuses, an ICC profile included.  A refused image gets its status in
 * statuses[i] and the others still encode.  An error on the device (EncoderStatus_OutOfMemory when the workspace of the batch does not
 * fit) fails every accepted image of the batch; the encoder stays usable.  Returns the first status that is not Ok; err then names the
 * image ("image 3: ...").  n == 0 returns Ok.  There are no progress callbacks and no cancellation, and the thread-local
 * jxlhip_last_save_* reporters are not touched. */
JXLFILETYPEIO_API EncoderStatus jxlhip_encode_batch(JxlHipEncoder* enc, int32_t n, const JxlHipPixels* images, const EncoderOptions* options,
                                                    const EncoderImageMetadata* const* metadata, EncoderStatus* statuses, ErrorInfo* err);

/* jxlhip_encode_batch with a JxlHipLossyOptions per image: lossy[i] belongs to images[i]; lossy may be NULL, meaning all zero
 * (jxlhip_encode_batch is this call with NULL).  The file of image i is, byte for byte, what jxlhip_save_pixels_lossy writes with
 * options[i] and lossy[i].  An image whose lossy[i] that call refuses is refused here the same way, in statuses[i]. */
JXLFILETYPEIO_API EncoderStatus jxlhip_encode_batch_lossy(JxlHipEncoder* enc, int32_t n, const JxlHipPixels* images, const EncoderOptions* options,
                                                          const JxlHipLossyOptions* lossy, const EncoderImageMetadata* const* metadata,
                                                          EncoderStatus* statuses, ErrorInfo* err);

/* The file of image i of the last batch: host memory owned by the encoder, valid until the next batch or destroy.  Returns 1, or 0
 * when there is none (an index outside the batch, a refused or failed image). */
JXLFILETYPEIO_API int32_t jxlhip_encoder_result(JxlHipEncoder* enc, int32_t i, const uint8_t** data, size_t* size);

/* Timing of the last batch, shaped like jxlhip_stage_times: device milliseconds per named stage (HIP events on the stream the stage
 * ran on; stages on different streams overlap), then the host's stages on the host clock, named "host: ...".  The stages that
 * allocate ("host: ... allocation") appear only in a call that had to grow a buffer. */
JXLFILETYPEIO_API int32_t jxlhip_encoder_stage_times(JxlHipEncoder* enc, const char** names, float* ms, int32_t capacity);

/* =====================================================================================================
 * Part 5: animations - every displayed image of a file, decoded to device memory (not in the reference, whose LoadImage
 * keeps the first displayed image; LoadImage and jxlhip_decode_batch still do exactly that).
 *
 * Displayed image j is the canvas after the j-th frame, in file order, that ends the file or has a duration.  Frames
 * without a duration between them are layers: they blend onto the canvas and may be saved to the four reference slots.
 * Those slots are the state between two displayed images, so decoding is sequential from an ENTRY POINT: image 0, or an
 * image in front of whose first frame no slot is alive (nothing written before it is read from there on).  jxlhip_animation_seek
 * resumes at the nearest one; an encoder's key frames (jxlhip_encode_animation, key_interval) are entry points.
 * A file without an animation header is accepted: a single frame or a layered still has one displayed image, the one
 * LoadImage delivers.  Files whose frames carry patches or are reference-only frames are refused by name at open
 * ("animations with patches are not supported"), and so is everything LoadImage refuses of a layered file, with the same
 * words and the number of the codestream frame.  There is no limit on the number of frames.
 * ===================================================================================================== */
typedef struct JxlHipAnimation JxlHipAnimation;

typedef struct JxlHipAnimationInfo {
  int32_t width, height;         /* as displayed (orientation applied), like jxlhip_peek */
  int32_t num_channels, has_alpha;
  int32_t bytes_per_sample;      /* 1, 2 or 4 */
  int32_t float_samples;         /* 1: binary16 / binary32 samples */
  int32_t bits_per_sample;       /* of the colour channels, as coded */
  int32_t have_animation;        /* 0: no animation header; the four fields below are 0 */
  uint32_t tps_numerator, tps_denominator;   /* ticks per second = numerator / denominator */
  uint32_t num_loops;            /* 0: endless */
  int32_t have_timecodes;
  int32_t num_displayed;         /* displayed images in the file */
  int32_t num_codestream_frames; /* frames in the file, layers included */
  uint64_t image_bytes;          /* one displayed image: width * height * num_channels * bytes_per_sample, tight rows */
} JxlHipAnimationInfo;

typedef struct JxlHipAnimationFrame {
  uint32_t duration;             /* ticks the image is shown for (0 for the only image of a still) */
  uint32_t timecode;             /* as written (have_timecodes), else 0 */
  int32_t first_codestream_frame, num_codestream_frames;   /* the frames consumed since the previous displayed image */
  int32_t name_length;           /* bytes of `name`, without the NUL */
  char name[1076];               /* the name of the frame that completes the image, NUL-terminated */
} JxlHipAnimationFrame;

/* Parses the whole file on the host (the bytes are copied: `data` may be freed after the call), then creates a decoder on
 * `device` (< 0: the current one) and uploads the codestream once.  info may be NULL.  Returns NULL on failure, message in err. */
JXLFILETYPEIO_API JxlHipAnimation* jxlhip_animation_open(int32_t device, const uint8_t* data, size_t size, JxlHipAnimationInfo* info,
                                                         ErrorInfo* err);
JXLFILETYPEIO_API void jxlhip_animation_close(JxlHipAnimation* anim);
/* Displayed image j (0 .. num_displayed - 1).  Returns 1, or 0 for an index outside the file. */
JXLFILETYPEIO_API int32_t jxlhip_animation_frame(JxlHipAnimation* anim, int32_t j, JxlHipAnimationFrame* out);
/* Writes the next `count` displayed images (fewer at the end of the file; 0 there), tightly packed, image_bytes each, into
 * the device buffer dev_out of `capacity` bytes; *written is how many.  Synchronous.  The frames are decoded in chunks of
 * consecutive codestream frames - at most 64, and at most 16 GiB of scratch unless one frame needs more - so the scratch
 * does not grow with the length of the file.  After a failure (the message names the codestream frame) the position and
 * the reference slots are those in front of the chunk that failed (a chunk stores its slots to a second set of buffers, which
 * becomes the state only when the chunk has succeeded): images in front of the damaged frame can still be asked for. */
JXLFILETYPEIO_API DecoderStatus jxlhip_animation_next(JxlHipAnimation* anim, int32_t count, void* dev_out, size_t capacity,
                                                      int32_t* written, ErrorInfo* err);
/* Back to the first displayed image: jxlhip_animation_seek(anim, 0). */
JXLFILETYPEIO_API void jxlhip_animation_rewind(JxlHipAnimation* anim);
/* The entry points, ascending displayed indices (image 0 is always one).  Returns how many there are and writes up to
 * `capacity` of them; displayed NULL or capacity 0: the count only. */
JXLFILETYPEIO_API int32_t jxlhip_animation_entry_points(JxlHipAnimation* anim, int32_t* displayed, int32_t capacity);
/* After it jxlhip_animation_next delivers displayed image j (j == num_displayed: the end; anything else outside the file:
 * InvalidParameter, position unchanged).  j equal to the position does nothing.  Otherwise decoding resumes at the latest
 * entry point e <= j - unless the decode stands in [e, j] already: a forward seek never goes back.  Nothing is decoded
 * by the call: the images between the resume point and j are decoded for the reference slots only (none of them is
 * stored, no buffer is needed for them), in the same chunks as the images asked for next. */
JXLFILETYPEIO_API DecoderStatus jxlhip_animation_seek(JxlHipAnimation* anim, int32_t j, ErrorInfo* err);
/* Where the next chunk starts (codestream frame) and which displayed image is delivered next.  Either pointer may be NULL. */
JXLFILETYPEIO_API void jxlhip_animation_position(JxlHipAnimation* anim, int32_t* next_codestream_frame, int32_t* next_displayed);
/* Thumbnails: with p the position, displayed images p, p + step, p + 2 step, ... (step >= 1) at 1:8, tightly packed into
 * dev_out - n = min(count, ceil((num_displayed - p) / step)) of them, *written says how many; the position afterwards is
 * min(num_displayed, p + n * step).  An image has ceil(width / 8) x ceil(height / 8) pixels, tight rows, the channels and
 * sample type of the full-size image; a sample is the mean over one 8 x 8 cell of the displayed (oriented) image of the
 * samples jxlhip_animation_next stores, cell (0, 0) at the top left, partial cells at the right and bottom edge averaging
 * the pixels that exist: integers (sum + n / 2) / n, binary16 / binary32 the float32 sum divided by n and rounded to the
 * type.  The images in between are decoded for the reference slots only.  Nothing is ever stored at full size.  A
 * capacity that is too small: InvalidParameter, with the byte counts.  Combines freely with next, seek and rewind. */
JXLFILETYPEIO_API DecoderStatus jxlhip_animation_next_reduced(JxlHipAnimation* anim, int32_t count, int32_t step, void* dev_out,
                                                              size_t capacity, int32_t* written, ErrorInfo* err);
/* "chunk_frames" (0: chunks by the limits above, the default; n >= 1: at most n frames per chunk - same output, for tests);
 * "lane_stride", "no_direct", "mod_lanes64", "no_stream_pairs" and "no_lf_pipeline" go to the animation's decoder as
 * jxlhip_set_option takes them (same output).  Every other name is refused: neither a band nor a reduced size is offered
 * here.  Returns 1 if the option was set. */
JXLFILETYPEIO_API int32_t jxlhip_animation_set_option(JxlHipAnimation* anim, const char* name, int32_t value);
/* The decoder the animation runs on, owned by it: for jxlhip_stage_times / jxlhip_stage_totals (measurement). */
JXLFILETYPEIO_API JxlHipDecoder* jxlhip_animation_decoder(JxlHipAnimation* anim);

/* =====================================================================================================
 * Part 6: animation encode - a stack of device-resident frames as ONE animated file (not in the reference).
 *
 * Frame 0 is written whole.  Every later frame is written as the bounding box of the samples whose bits differ from its
 * predecessor's (measured on the GPU, in the caller's memory), replacing that part of the canvas: lossless frames as the
 * exact box, lossy frames as the box grown outwards to multiples of 8 canvas pixels (clipped to the canvas).  A frame that
 * equals its predecessor is written as the 1 x 1 rectangle at (0, 0): the file has one displayed image per input frame, and
 * durations are never merged.  Every frame replaces (colour and alpha), reads and is saved to reference slot 1, and has no
 * name; there are no timecodes.
 * ===================================================================================================== */
typedef struct JxlHipAnimationOptions {
  uint32_t tps_numerator, tps_denominator;   /* ticks per second = numerator / denominator; numerator 1 .. 2^30, denominator 1 .. 1024 */
  uint32_t num_loops;                        /* 0: endless */
  int32_t key_interval;                      /* >= 1: every key_interval-th frame is written whole, like frame 0 (an entry point that
                                              * needs no earlier frame); <= 0: only frame 0 */
  int32_t chunk_frames;                      /* >= 1: at most this many frames go through the encoder at a time; <= 0: as many as a
                                              * workspace of 32 GiB holds, at most 64.  The file's bytes do not depend on it */
} JxlHipAnimationOptions;

/* Encodes n frames (frames[k].data: DEVICE pointers, as for jxlhip_encode_batch; only read) into one file, read with
 * jxlhip_encoder_result(enc, 0, ...).  durations[k]: ticks frame k is shown for, >= 1.  `options` holds for every frame.  metadata
 * may be NULL (Exif and XMP: host pointers, written once).  Synchronous.
 * The bytes of frame k from its TOC on are those of jxlhip_save_pixels for the frame's rectangle with the same options.
 * Refused on the host, before any device work, with EncoderStatus_EncodeError and a message: whatever jxlhip_encode_batch refuses
 * of an image (in the same words, behind "frame k: "), n < 1, frames that differ from frame 0 in size, channels, sample type,
 * bits or colour, a duration of 0, and ticks per second outside their ranges.  After a failure, refusals included, the encoder
 * holds no result and stays usable. */
JXLFILETYPEIO_API EncoderStatus jxlhip_encode_animation(JxlHipEncoder* enc, int32_t n, const JxlHipPixels* frames, const uint32_t* durations,
                                                        const EncoderOptions* options, const JxlHipAnimationOptions* animation,
                                                        const EncoderImageMetadata* metadata, ErrorInfo* err);

/* The rectangles of the last jxlhip_encode_animation that got as far as measuring them: x, y, width, height per frame, up to
 * `capacity` frames are written to xywh.  Returns the number of frames (0: none). */
JXLFILETYPEIO_API int32_t jxlhip_encoder_animation_rects(JxlHipEncoder* enc, int32_t* xywh, int32_t capacity);

/* Several rectangles per frame.  A frame that changed in two far-apart places has a bounding box as large as the canvas; with
 * max_rects >= 2 what changed is measured per 64 x 64-pixel tile instead, and a frame that is no key frame is written as up to
 * max_rects pairwise disjoint rectangles that together cover every changed pixel: the 8-connected groups of changed tiles, their
 * boxes (lossy: on the 8-pixel grid) merged where they overlap, then the cheapest pair - the one whose common box adds the fewest
 * pixels - merged while there are more than max_rects or while that costs at most merge_pixels (DESIGN.md §2 "Animation encode"
 * states the rule in full).  A frame with m rectangles is m frames of the codestream, each replacing its part of slot 1: the first
 * m - 1 have duration 0, so that a decoder composes them into the displayed image that the last, with the frame's duration, ends.
 * The file still has one displayed image per input frame.  chunk_frames and its limits count codestream frames. */
typedef struct JxlHipAnimationRectOptions {
  int32_t max_rects;     /* 1: one rectangle per frame, byte for byte jxlhip_encode_animation; 2..16: up to this many */
  int32_t merge_pixels;  /* two rectangles become one when that codes at most this many pixels more; >= 0 */
} JxlHipAnimationRectOptions;

/* jxlhip_encode_animation with `rects` (jxlhip_encode_animation is this call with {1, 0}).  Refused in addition, on the host and in
 * words: max_rects outside 1..16 and a negative merge_pixels. */
JXLFILETYPEIO_API EncoderStatus jxlhip_encode_animation_rects(JxlHipEncoder* enc, int32_t n, const JxlHipPixels* frames, const uint32_t* durations,
                                                              const EncoderOptions* options, const JxlHipAnimationOptions* animation,
                                                              const JxlHipAnimationRectOptions* rects, const EncoderImageMetadata* metadata,
                                                              ErrorInfo* err);

/* The codestream frames of the last animation that got as far as measuring: input frame, x, y, width, height per codestream frame, in
 * file order; up to `capacity` of them are written to kxywh.  Returns their number.  (jxlhip_encoder_animation_rects keeps reporting
 * one rectangle per input frame: the bounding box of the frame's rectangles, the same value for every max_rects.) */
JXLFILETYPEIO_API int32_t jxlhip_encoder_animation_frame_rects(JxlHipEncoder* enc, int32_t* kxywh, int32_t capacity);

/* The tile table of pair `pair` (frames pair and pair + 1) of the last animation encoded with max_rects >= 2: one word per 64 x 64 tile,
 * row-major over ceil(width / 64) x ceil(height / 64) tiles, holding the bytes x0, y0, x1, y1 (lowest first; inclusive, relative to the
 * tile's origin) of the box of the changed pixels in the tile, 0xFFFFFFFF where none changed.  Up to `capacity` words are written to
 * dst.  Returns the number of tiles (0: no such pair, or max_rects was 1 and there was no tolerance).
 * With a tolerance > 0 (jxlhip_encode_animation_changes) it is the table of frame pair + 1 against the reference canvas as it stood before
 * that frame, and there is one for every pair whatever max_rects is, key frames included (a key frame is measured, then written whole). */
JXLFILETYPEIO_API int32_t jxlhip_encoder_animation_tiles(JxlHipEncoder* enc, int32_t pair, uint32_t* dst, int32_t capacity);

/* A tolerance for "unchanged".  The bits decide above, so one count of sensor noise per sample makes every frame be written whole.
 * With tolerance > 0 a frame is compared not with its predecessor but with what a decoder SHOWS: the encoder keeps a reference canvas R
 * on the device (tight rows, the frames' pixel format), which starts as frame 0.  For k = 1 .. n - 1 in order: the tile table of frame k
 * against R is measured; the rectangles follow from it by the rules above (max_rects = 1: the table's bounding box; a key frame: the
 * canvas); then R takes frame k's pixels inside each of those rectangles - the 1 x 1 rectangle of a frame in which nothing changed and,
 * for lossy frames, the rectangles grown to the 8-pixel grid included: the pixels a decoder replaces.  So R is the source of exactly
 * what is shown, and before coding error no displayed sample is further than the tolerance from its source sample, in any frame (a
 * tolerance against the predecessor would let a slow fade drift without bound).  The rectangles are still coded from the caller's frame
 * k; headers, slots, durations and chunking are as above.
 * The tolerance holds for every sample of every channel, alpha included.  A pixel is changed when one of its samples is:
 *  - integer samples: changed when |a - b| > floor(tolerance), on the stored values (bits_per_sample plays no part);
 *  - binary16 / binary32: unchanged when the bit patterns are equal, or when both values are finite and |a - b| <= tolerance, the
 *    subtraction in binary32 (binary16 widened first); changed otherwise.  So +0 and -0 are unchanged, equal NaN patterns are, and a NaN
 *    or an infinity against anything else is changed.
 * tolerance == 0 is jxlhip_encode_animation_rects byte for byte (the bit rule against the predecessor, measured in one launch).
 * Lossless is allowed together with a tolerance: every coded rectangle is exact and the rest of the canvas is within the tolerance of
 * its source - the file is no longer a lossless copy of the frames. */
typedef struct JxlHipAnimationChangeOptions {
  float tolerance;       /* >= 0 and finite; 0: the bits decide */
} JxlHipAnimationChangeOptions;

/* jxlhip_encode_animation_rects with `changes` (jxlhip_encode_animation_rects is this call with {0}).  Refused in addition, on the host,
 * in words and before any device work: a negative, NaN or infinite tolerance. */
JXLFILETYPEIO_API EncoderStatus jxlhip_encode_animation_changes(JxlHipEncoder* enc, int32_t n, const JxlHipPixels* frames, const uint32_t* durations,
                                                                const EncoderOptions* options, const JxlHipAnimationOptions* animation,
                                                                const JxlHipAnimationRectOptions* rects, const JxlHipAnimationChangeOptions* changes,
                                                                const EncoderImageMetadata* metadata, ErrorInfo* err);

#ifdef __cplusplus
}
static_assert(sizeof(JxlHipPixels) == 40, "JxlHipPixels layout");
static_assert(sizeof(JxlHipLossyOptions) == 16, "JxlHipLossyOptions layout");
static_assert(sizeof(JxlHipAnimationOptions) == 20, "JxlHipAnimationOptions layout");
static_assert(sizeof(JxlHipAnimationRectOptions) == 8, "JxlHipAnimationRectOptions layout");
static_assert(sizeof(JxlHipAnimationChangeOptions) == 4, "JxlHipAnimationChangeOptions layout");
static_assert(sizeof(JxlHipAnimationInfo) == 64, "JxlHipAnimationInfo layout");
static_assert(sizeof(JxlHipAnimationFrame) == 1096, "JxlHipAnimationFrame layout");
static_assert(sizeof(BitmapData) == 24, "BitmapData layout");
static_assert(sizeof(EncoderOptions) == 12, "EncoderOptions layout");
static_assert(sizeof(EncoderImageMetadata) == 48, "EncoderImageMetadata layout");
static_assert(sizeof(IOCallbacks) == 16, "IOCallbacks layout");
static_assert(sizeof(ErrorInfo) == 256, "ErrorInfo layout");
static_assert(sizeof(DecoderCallbacks) == 48, "DecoderCallbacks layout");
static_assert(sizeof(bool) == 1, "bool is one byte across the boundary");
#endif

#endif /* JXLFILETYPEIO_H_ */
