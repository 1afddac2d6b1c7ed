"""Host-side mirror of the reference's managed interop (src/Interop/JpegXLNative.cs) over ctypes.

`load_image` / `save_image` / `get_libjxl_version` call the three C-ABI exports exactly like the C# host
does (callback struct of six function pointers, ErrorInfo, status -> exception mapping).  `Decoder` wraps the
device-resident batch entry points used by bench.py and the GPU parity tests, `Encoder` the device-resident batch encode.

The native library must exist: there is no CPU fallback.  Build it with `python -m pdn_jpegxl_amd.build`.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

# ---------------------------------------------------------------- enums (include/jxlfiletypeio.h)
DECODER_STATUS = ["Ok", "NullParameter", "InvalidParameter", "OutOfMemory", "HasAnimation", "HasMultipleFrames",
                  "ImageDimensionExceedsInt32", "UnsupportedChannelFormat", "CreateLayerError", "CreateMetadataError",
                  "DecodeError", "MetadataError", "InvalidFileSignature"]
ENCODER_STATUS = ["Ok", "NullParameter", "OutOfMemory", "UserCanceled", "EncodeError", "WriteError"]
IMAGE_FORMAT = ["Gray", "Rgb", "Cmyk"]
KNOWN_PROFILE = ["Srgb", "LinearSrgb", "LinearGray", "GraySrgbTRC", "DisplayP3", "Rec709", "Rec2020Linear", "Rec2020PQ"]
S_OK, E_ABORT, E_OUTOFMEMORY, E_FAIL = 0, -2147467260, -2147024882, -2147467259


class ErrorInfo(C.Structure):
    _fields_ = [("errorMessage", C.c_char * 256)]


class BitmapData(C.Structure):
    _fields_ = [("scan0", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("stride", C.c_uint32)]


class EncoderOptions(C.Structure):
    _fields_ = [("distance", C.c_float), ("effort", C.c_int32), ("lossless", C.c_bool)]


class EncoderImageMetadata(C.Structure):
    _fields_ = [("exif", C.c_void_p), ("exifSize", C.c_size_t), ("iccProfile", C.c_void_p), ("iccProfileSize", C.c_size_t),
                ("xmp", C.c_void_p), ("xmpSize", C.c_size_t)]


SetBasicInfoFn = C.CFUNCTYPE(None, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_bool)
SetMetadataFn = C.CFUNCTYPE(C.c_bool, C.POINTER(C.c_uint8), C.c_size_t)
SetKnownProfileFn = C.CFUNCTYPE(C.c_bool, C.c_int32)
SetLayerDataFn = C.CFUNCTYPE(C.c_bool, C.POINTER(C.c_uint8), C.c_void_p, C.c_size_t)
WriteFn = C.CFUNCTYPE(C.c_int32, C.POINTER(C.c_uint8), C.c_size_t)
SeekFn = C.CFUNCTYPE(C.c_int32, C.c_uint64)
ProgressFn = C.CFUNCTYPE(C.c_bool, C.c_int32)


class DecoderCallbacks(C.Structure):
    _fields_ = [("setBasicInfo", SetBasicInfoFn), ("setIccProfile", SetMetadataFn), ("setKnownColorProfile", SetKnownProfileFn),
                ("setExif", SetMetadataFn), ("setXmp", SetMetadataFn), ("setLayerData", SetLayerDataFn)]


class IOCallbacks(C.Structure):
    _fields_ = [("Write", WriteFn), ("Seek", SeekFn)]


class ImageInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("num_channels", C.c_int32), ("has_alpha", C.c_int32),
                ("xsize_blocks", C.c_int32), ("ysize_blocks", C.c_int32), ("num_groups", C.c_int32), ("num_lf_groups", C.c_int32),
                ("epf_iters", C.c_int32), ("gaborish", C.c_int32), ("codestream_bytes", C.c_uint64), ("bytes_per_sample", C.c_int32),
                ("reserved", C.c_int32)]


class LosslessInfo(C.Structure):
    _fields_ = [("tier", C.c_int32), ("palette_colours", C.c_int32), ("rct_type", C.c_int32), ("num_channels", C.c_int32),
                ("predictor", C.c_int32 * 4), ("leaves", C.c_int32), ("clusters", C.c_int32), ("fell_back_to_effort7", C.c_int32),
                ("reserved", C.c_int32), ("searched_bytes", C.c_uint64), ("effort7_bytes", C.c_uint64)]


class JxlHipPixels(C.Structure):
    _fields_ = [("data", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("stride_bytes", C.c_uint64),
                ("num_channels", C.c_int32), ("sample_type", C.c_int32), ("bits_per_sample", C.c_int32), ("colour", C.c_int32)]


class JxlHipLossyOptions(C.Structure):
    _fields_ = [("chroma_from_luma", C.c_int32), ("reserved", C.c_int32 * 3)]


def _lossy_options(cfl):
    """cfl: False / True (chroma-from-luma maps all zero / fitted per tile), or a JxlHipLossyOptions as it is."""
    return cfl if isinstance(cfl, JxlHipLossyOptions) else JxlHipLossyOptions(int(cfl))


class AnimationOptions(C.Structure):
    _fields_ = [("tps_numerator", C.c_uint32), ("tps_denominator", C.c_uint32), ("num_loops", C.c_uint32), ("key_interval", C.c_int32),
                ("chunk_frames", C.c_int32)]


class AnimationRectOptions(C.Structure):
    _fields_ = [("max_rects", C.c_int32), ("merge_pixels", C.c_int32)]


class AnimationChangeOptions(C.Structure):
    _fields_ = [("tolerance", C.c_float)]


class AnimationInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("num_channels", C.c_int32), ("has_alpha", C.c_int32),
                ("bytes_per_sample", C.c_int32), ("float_samples", C.c_int32), ("bits_per_sample", C.c_int32), ("have_animation", C.c_int32),
                ("tps_numerator", C.c_uint32), ("tps_denominator", C.c_uint32), ("num_loops", C.c_uint32), ("have_timecodes", C.c_int32),
                ("num_displayed", C.c_int32), ("num_codestream_frames", C.c_int32), ("image_bytes", C.c_uint64)]


class AnimationFrame(C.Structure):
    _fields_ = [("duration", C.c_uint32), ("timecode", C.c_uint32), ("first_codestream_frame", C.c_int32),
                ("num_codestream_frames", C.c_int32), ("name_length", C.c_int32), ("name", C.c_char * 1076)]


EXPORTS = ["GetLibJxlVersion", "LoadImage", "SaveImage", "jxlhip_parse_icc", "jxlhip_decoder_create", "jxlhip_decoder_destroy", "jxlhip_peek",
           "jxlhip_decode_batch", "jxlhip_finish", "jxlhip_read_plane", "jxlhip_set_option", "jxlhip_stage_times", "jxlhip_stage_totals",
           "jxlhip_last_load_stage_times", "jxlhip_last_save_stage_times", "jxlhip_distance_map", "jxlhip_last_save_distances",
           "jxlhip_last_save_lossless_info", "jxlhip_save_pixels", "jxlhip_save_pixels_lossy", "jxlhip_encoder_create", "jxlhip_encoder_destroy",
           "jxlhip_encode_batch", "jxlhip_encode_batch_lossy",
           "jxlhip_encoder_result", "jxlhip_encoder_stage_times", "jxlhip_encode_animation", "jxlhip_encoder_animation_rects", "jxlhip_encode_animation_rects",
           "jxlhip_encoder_animation_frame_rects", "jxlhip_encoder_animation_tiles", "jxlhip_encode_animation_changes", "jxlhip_animation_open", "jxlhip_animation_close", "jxlhip_animation_frame",
           "jxlhip_animation_next", "jxlhip_animation_rewind", "jxlhip_animation_set_option", "jxlhip_animation_decoder", "jxlhip_animation_entry_points",
           "jxlhip_animation_seek", "jxlhip_animation_position", "jxlhip_animation_next_reduced"]

_lib = None


_selftest_lib = None


def selftest_lib():
    """The TEST library (the product's objects + csrc/selftest.cc): writer self tests for the CPU suite.  The production library
    does not export these hooks."""
    global _selftest_lib
    if _selftest_lib is None:
        lib()   # builds if needed, checks the manifest, loads torch's HIP runtime first
        _selftest_lib = C.CDLL(_build.test_lib_path())
    return _selftest_lib


class NativeLibraryMissing(RuntimeError):
    pass


def lib(build_if_missing=True):
    """Loads the native library; raises NativeLibraryMissing if it cannot be built/loaded (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        # When PyTorch is present it must load first: both link libamdhip64.so.7 and have to share ONE HIP runtime
        # (torch bundles its own); loading the system runtime first leaves torch without a visible GPU.
        import torch  # noqa: F401
    except ImportError:
        pass
    path = _build.lib_path()
    if not os.path.exists(path):
        if not build_if_missing:
            raise NativeLibraryMissing(path)
        _build.build()
    # a library built from other sources than the ones in the tree is refused, not used (and not rebuilt here: this process may already
    # hold the GPU, e.g. under a profiler)
    try:
        built_from = open(_build.manifest_path()).read()
    except OSError:
        built_from = None
    if built_from != _build.manifest_text():
        raise NativeLibraryMissing("%s is stale (built from different sources): run python -m pdn_jpegxl_amd.build" % path)
    try:
        L = C.CDLL(path)
    except OSError as e:
        raise NativeLibraryMissing("%s: %s" % (path, e))
    L.GetLibJxlVersion.restype = C.c_uint32
    L.LoadImage.restype = C.c_int32
    L.LoadImage.argtypes = [C.POINTER(DecoderCallbacks), C.c_char_p, C.c_size_t, C.POINTER(ErrorInfo)]
    L.SaveImage.restype = C.c_int32
    L.SaveImage.argtypes = [C.POINTER(BitmapData), C.POINTER(EncoderOptions), C.POINTER(EncoderImageMetadata), C.POINTER(IOCallbacks),
                            C.POINTER(ErrorInfo), ProgressFn]
    L.jxlhip_decoder_create.restype = C.c_void_p
    L.jxlhip_decoder_create.argtypes = [C.c_int32, C.POINTER(ErrorInfo)]
    L.jxlhip_decoder_destroy.argtypes = [C.c_void_p]
    L.jxlhip_peek.restype = C.c_int32
    L.jxlhip_peek.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(ImageInfo), C.POINTER(ErrorInfo)]
    L.jxlhip_decode_batch.restype = C.c_int32
    L.jxlhip_decode_batch.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_void_p), C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(ErrorInfo)]
    L.jxlhip_finish.restype = C.c_int32
    L.jxlhip_finish.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(ErrorInfo)]
    L.jxlhip_read_plane.restype = C.c_size_t
    L.jxlhip_read_plane.argtypes = [C.c_void_p, C.c_int32, C.c_char_p, C.c_int32, C.c_void_p, C.c_size_t]
    L.jxlhip_set_option.restype = C.c_int32
    L.jxlhip_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
    L.jxlhip_stage_times.restype = C.c_int32
    L.jxlhip_stage_times.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int32]
    L.jxlhip_stage_totals.restype = C.c_int32
    L.jxlhip_stage_totals.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_int32), C.c_int32]
    L.jxlhip_distance_map.restype = C.c_int32
    L.jxlhip_distance_map.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                      C.POINTER(ErrorInfo)]
    L.jxlhip_last_save_distances.restype = C.c_size_t
    L.jxlhip_last_save_distances.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                             C.POINTER(C.c_int32)]
    L.jxlhip_last_save_lossless_info.restype = None
    L.jxlhip_last_save_lossless_info.argtypes = [C.POINTER(LosslessInfo)]
    L.jxlhip_save_pixels.restype = C.c_int32
    L.jxlhip_save_pixels.argtypes = [C.POINTER(JxlHipPixels), C.POINTER(EncoderOptions), C.POINTER(EncoderImageMetadata),
                                     C.POINTER(IOCallbacks), C.POINTER(ErrorInfo), ProgressFn]
    L.jxlhip_save_pixels_lossy.restype = C.c_int32
    L.jxlhip_save_pixels_lossy.argtypes = [C.POINTER(JxlHipPixels), C.POINTER(EncoderOptions), C.POINTER(JxlHipLossyOptions),
                                           C.POINTER(EncoderImageMetadata), C.POINTER(IOCallbacks), C.POINTER(ErrorInfo), ProgressFn]
    L.jxlhip_encoder_create.restype = C.c_void_p
    L.jxlhip_encoder_create.argtypes = [C.c_int32, C.POINTER(ErrorInfo)]
    L.jxlhip_encoder_destroy.restype = None
    L.jxlhip_encoder_destroy.argtypes = [C.c_void_p]
    L.jxlhip_encode_batch.restype = C.c_int32
    L.jxlhip_encode_batch.argtypes = [C.c_void_p, C.c_int32, C.POINTER(JxlHipPixels), C.POINTER(EncoderOptions),
                                      C.POINTER(C.POINTER(EncoderImageMetadata)), C.POINTER(C.c_int32), C.POINTER(ErrorInfo)]
    L.jxlhip_encode_batch_lossy.restype = C.c_int32
    L.jxlhip_encode_batch_lossy.argtypes = [C.c_void_p, C.c_int32, C.POINTER(JxlHipPixels), C.POINTER(EncoderOptions), C.POINTER(JxlHipLossyOptions),
                                            C.POINTER(C.POINTER(EncoderImageMetadata)), C.POINTER(C.c_int32), C.POINTER(ErrorInfo)]
    L.jxlhip_encoder_result.restype = C.c_int32
    L.jxlhip_encoder_result.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.jxlhip_encoder_stage_times.restype = C.c_int32
    L.jxlhip_encoder_stage_times.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int32]
    L.jxlhip_encode_animation.restype = C.c_int32
    L.jxlhip_encode_animation.argtypes = [C.c_void_p, C.c_int32, C.POINTER(JxlHipPixels), C.POINTER(C.c_uint32), C.POINTER(EncoderOptions),
                                          C.POINTER(AnimationOptions), C.POINTER(EncoderImageMetadata), C.POINTER(ErrorInfo)]
    L.jxlhip_encoder_animation_rects.restype = C.c_int32
    L.jxlhip_encoder_animation_rects.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32]
    L.jxlhip_encode_animation_rects.restype = C.c_int32
    L.jxlhip_encode_animation_rects.argtypes = [C.c_void_p, C.c_int32, C.POINTER(JxlHipPixels), C.POINTER(C.c_uint32), C.POINTER(EncoderOptions),
                                                C.POINTER(AnimationOptions), C.POINTER(AnimationRectOptions), C.POINTER(EncoderImageMetadata),
                                                C.POINTER(ErrorInfo)]
    L.jxlhip_encode_animation_changes.restype = C.c_int32
    L.jxlhip_encode_animation_changes.argtypes = [C.c_void_p, C.c_int32, C.POINTER(JxlHipPixels), C.POINTER(C.c_uint32), C.POINTER(EncoderOptions),
                                                  C.POINTER(AnimationOptions), C.POINTER(AnimationRectOptions), C.POINTER(AnimationChangeOptions),
                                                  C.POINTER(EncoderImageMetadata), C.POINTER(ErrorInfo)]
    L.jxlhip_encoder_animation_frame_rects.restype = C.c_int32
    L.jxlhip_encoder_animation_frame_rects.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32]
    L.jxlhip_encoder_animation_tiles.restype = C.c_int32
    L.jxlhip_encoder_animation_tiles.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_uint32), C.c_int32]
    L.jxlhip_animation_open.restype = C.c_void_p
    L.jxlhip_animation_open.argtypes = [C.c_int32, C.c_char_p, C.c_size_t, C.POINTER(AnimationInfo), C.POINTER(ErrorInfo)]
    L.jxlhip_animation_close.restype = None
    L.jxlhip_animation_close.argtypes = [C.c_void_p]
    L.jxlhip_animation_frame.restype = C.c_int32
    L.jxlhip_animation_frame.argtypes = [C.c_void_p, C.c_int32, C.POINTER(AnimationFrame)]
    L.jxlhip_animation_next.restype = C.c_int32
    L.jxlhip_animation_next.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(ErrorInfo)]
    L.jxlhip_animation_rewind.restype = None
    L.jxlhip_animation_rewind.argtypes = [C.c_void_p]
    L.jxlhip_animation_entry_points.restype = C.c_int32
    L.jxlhip_animation_entry_points.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32]
    L.jxlhip_animation_seek.restype = C.c_int32
    L.jxlhip_animation_seek.argtypes = [C.c_void_p, C.c_int32, C.POINTER(ErrorInfo)]
    L.jxlhip_animation_position.restype = None
    L.jxlhip_animation_position.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.jxlhip_animation_next_reduced.restype = C.c_int32
    L.jxlhip_animation_next_reduced.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(ErrorInfo)]
    L.jxlhip_animation_set_option.restype = C.c_int32
    L.jxlhip_animation_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
    L.jxlhip_animation_decoder.restype = C.c_void_p
    L.jxlhip_animation_decoder.argtypes = [C.c_void_p]
    L.jxlhip_parse_check.restype = C.c_int32
    L.jxlhip_parse_check.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(ErrorInfo)]
    L.jxlhip_static_table.restype = C.c_size_t
    L.jxlhip_static_table.argtypes = [C.c_char_p, C.c_int32, C.c_void_p, C.c_size_t]
    _lib = L
    return L


# ---------------------------------------------------------------- exceptions (JpegXLNative.cs:128-239)
class JxlError(RuntimeError):
    def __init__(self, status, message=""):
        self.status = status
        super().__init__("%s%s" % (status, (": " + message) if message else ""))


class FormatError(JxlError):
    pass


def get_libjxl_version():
    """(major, minor, patch) as JpegXLNative.GetLibJxlVersion unpacks it (JpegXLNative.cs:40-42)."""
    v = lib().GetLibJxlVersion()
    return (v >> 24) & 0xFF, (v >> 16) & 0xFF, (v >> 8) & 0xFF


class DecodedImage:
    """What the host's DecoderImage sink collects (src/Interop/DecoderImage.cs)."""

    def __init__(self):
        self.width = self.height = 0
        self.format = None
        self.channel_representation = 0
        self.has_transparency = False
        self.known_profile = None
        self.icc = None
        self.exif = None
        self.xmp = None
        self.pixels = None
        self.layer_name = None
        self.trace = []


def load_image(data, fail_at=None):
    """JpegXLNative.LoadImage: data = whole file (bytes).  Returns DecodedImage.  `fail_at` makes the named callback
    return false (host-side failure injection, e.g. 'setLayerData')."""
    L = lib()
    img = DecodedImage()

    def basic(w, h, fmt, rep, alpha):
        img.trace.append("setBasicInfo")
        img.width, img.height, img.format, img.channel_representation, img.has_transparency = w, h, IMAGE_FORMAT[fmt], rep, bool(alpha)

    def icc(p, n):
        img.trace.append("setIccProfile")
        img.icc = bytes(C.string_at(p, n))
        return fail_at != "setIccProfile"

    def known(p):
        img.trace.append("setKnownColorProfile")
        img.known_profile = KNOWN_PROFILE[p]
        return fail_at != "setKnownColorProfile"

    def exif(p, n):
        img.trace.append("setExif")
        img.exif = bytes(C.string_at(p, n))
        return fail_at != "setExif"

    def xmp(p, n):
        img.trace.append("setXmp")
        if img.xmp is None:  # the host keeps the first (DecoderImage.cs:248)
            img.xmp = bytes(C.string_at(p, n))
        return fail_at != "setXmp"

    def layer(p, name, nlen):
        img.trace.append("setLayerData")
        if fail_at == "setLayerData":
            return False
        nch = {"Gray": 1, "Rgb": 3, "Cmyk": 4}[img.format] + (1 if img.has_transparency else 0)
        n = img.width * img.height * nch
        # ImageChannelRepresentation (Common.h:33-39): Uint8, Uint16, Float16, Float32
        dt = (np.uint8, np.uint16, np.float16, np.float32)[img.channel_representation]
        nbytes = n * np.dtype(dt).itemsize
        img.pixels = np.ctypeslib.as_array(p, shape=(nbytes,)).view(dt).reshape(img.height, img.width, nch).copy()
        img.layer_name = C.string_at(name, nlen - 1).decode("utf-8", "replace") if name and nlen else None
        return True

    cbs = DecoderCallbacks(SetBasicInfoFn(basic), SetMetadataFn(icc), SetKnownProfileFn(known), SetMetadataFn(exif), SetMetadataFn(xmp),
                           SetLayerDataFn(layer))
    err = ErrorInfo()
    st = L.LoadImage(C.byref(cbs), data, len(data), C.byref(err))
    if st != 0:
        name = DECODER_STATUS[st] if 0 <= st < len(DECODER_STATUS) else str(st)
        msg = err.errorMessage.decode("ascii", "replace")
        if name in ("InvalidFileSignature", "DecodeError", "MetadataError", "HasAnimation", "HasMultipleFrames", "UnsupportedChannelFormat",
                    "ImageDimensionExceedsInt32"):
            raise FormatError(name, msg)
        raise JxlError(name, msg)
    return img


def save_image(bgra, distance=1.0, effort=7, lossless=False, exif=None, icc=None, xmp=None, progress=None, write_result=None):
    """JpegXLNative.SaveImage: bgra = uint8 (h, w, 4) BGRA surface (rows may be strided).  Returns the encoded bytes.
    write_result: HRESULT the Write callback returns instead of S_OK (failure injection)."""
    L = lib()
    bgra = np.asarray(bgra, dtype=np.uint8)
    if bgra.strides[2] != 1 or (bgra.shape[1] > 1 and bgra.strides[1] != 4):
        bgra = np.ascontiguousarray(bgra)
    h, w, _ = bgra.shape
    out = bytearray()
    pos = [0]

    def write(p, n):
        if write_result is not None:
            return write_result - (1 << 32) if write_result >= (1 << 31) else write_result
        chunk = C.string_at(p, n)
        end = pos[0] + n
        if end > len(out):
            out.extend(b"\0" * (end - len(out)))
        out[pos[0]:end] = chunk
        pos[0] = end
        return S_OK

    def seek(p):
        pos[0] = p
        return S_OK

    # numpy leaves the stride of a dimension of size 1 free (a contiguous 1 x 1 array may report 1): one row is w * 4 bytes apart
    bmp = BitmapData(bgra.ctypes.data, w, h, bgra.strides[0] if h > 1 else w * 4)
    opt = EncoderOptions(distance, effort, lossless)
    keep = [np.frombuffer(b, np.uint8) if b else None for b in (exif, icc, xmp)]
    md = EncoderImageMetadata(*sum(([k.ctypes.data if k is not None else None, len(k) if k is not None else 0] for k in keep), []))
    io = IOCallbacks(WriteFn(write), SeekFn(seek))
    err = ErrorInfo()
    st = L.SaveImage(C.byref(bmp), C.byref(opt), C.byref(md), C.byref(io), C.byref(err), ProgressFn(progress) if progress else ProgressFn())
    if st != 0:
        raise JxlError(ENCODER_STATUS[st] if 0 <= st < len(ENCODER_STATUS) else str(st), err.errorMessage.decode("ascii", "replace"))
    return bytes(out)


_SAMPLE_TYPES = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float16): 2, np.dtype(np.float32): 3}


def save_pixels(px, distance=1.0, effort=7, lossless=False, colour="Srgb", bits=None, exif=None, xmp=None, progress=None, cfl=False):
    """jxlhip_save_pixels_lossy: px = numpy array (h, w[, c]) of uint8, uint16, float16 or float32, c = 1..4 (Gray | Gray,A | R,G,B |
    R,G,B,A; rows may be strided).  colour: a KNOWN_PROFILE name, the space the samples are already in.  bits: of integer samples
    (default 8 for uint8, 16 for uint16; uint16 samples use the low `bits` bits).  cfl: True fits the chroma-from-luma maps of a lossy
    save per tile, False (the file of jxlhip_save_pixels) leaves them zero; a JxlHipLossyOptions is passed as it is; None calls
    jxlhip_save_pixels, the entry point without the struct.  Returns the encoded bytes."""
    L = lib()
    px = np.asarray(px)
    if px.dtype not in _SAMPLE_TYPES:
        raise ValueError("samples are uint8, uint16, float16 or float32")
    if px.ndim == 2:
        px = px[:, :, None]
    if px.ndim != 3:
        raise ValueError("a (h, w[, c]) array is expected")
    h, w, c = px.shape
    item = px.dtype.itemsize
    if px.strides[2] != item or (w > 1 and px.strides[1] != c * item) or (h > 1 and px.strides[0] < w * c * item):
        px = np.ascontiguousarray(px)
    if bits is None:
        bits = {1: 8, 2: 16}[item] if px.dtype.kind == "u" else 0
    out = bytearray()

    def write(p, n):
        out.extend(C.string_at(p, n))
        return S_OK

    desc = JxlHipPixels(px.ctypes.data, w, h, px.strides[0] if h > 1 else w * c * item, c, _SAMPLE_TYPES[px.dtype], bits,
                        KNOWN_PROFILE.index(colour))
    opt = EncoderOptions(distance, effort, lossless)
    keep = [np.frombuffer(b, np.uint8) if b else None for b in (exif, None, xmp)]
    md = EncoderImageMetadata(*sum(([k.ctypes.data if k is not None else None, len(k) if k is not None else 0] for k in keep), []))
    io = IOCallbacks(WriteFn(write), SeekFn(lambda p: S_OK))
    err = ErrorInfo()
    pf = ProgressFn(progress) if progress else ProgressFn()
    if cfl is None:
        st = L.jxlhip_save_pixels(C.byref(desc), C.byref(opt), C.byref(md), C.byref(io), C.byref(err), pf)
    else:
        st = L.jxlhip_save_pixels_lossy(C.byref(desc), C.byref(opt), C.byref(_lossy_options(cfl)), C.byref(md), C.byref(io), C.byref(err), pf)
    if st != 0:
        raise JxlError(ENCODER_STATUS[st] if 0 <= st < len(ENCODER_STATUS) else str(st), err.errorMessage.decode("ascii", "replace"))
    return bytes(out)


def peek(data):
    info, err = ImageInfo(), ErrorInfo()
    st = lib().jxlhip_peek(data, len(data), C.byref(info), C.byref(err))
    if st != 0:
        raise FormatError(DECODER_STATUS[st], err.errorMessage.decode("ascii", "replace"))
    return info


def reduced_size(width, height, factor):
    """(width, height) of an image decoded with the decoder option "downscale" = factor (1 or 8): one pixel per factor x factor cell,
    a partial cell at the right / bottom edge included.  width, height: the image as displayed, i.e. as `peek` reports it (sides
    already swapped for orientations 5..8); so is the result."""
    if factor not in (1, 8):
        raise ValueError("downscale factors are 1 and 8")
    return (int(width) + factor - 1) // factor, (int(height) + factor - 1) // factor


def parse_check(data):
    facts = (C.c_int32 * 8)()
    err = ErrorInfo()
    st = lib().jxlhip_parse_check(data, len(data), facts, C.byref(err))
    return DECODER_STATUS[st], list(facts), err.errorMessage.decode("ascii", "replace")


def parse_metadata(data, which):
    """Host-only: the Exif payload (which = 0) or the k-th `xml ` payload (which = k >= 1) as LoadImage would report it
    (Brotli-compressed `brob` boxes already decompressed); None if absent.  Returns (status, payload, message)."""
    L = lib()
    L.jxlhip_parse_metadata.restype = C.c_size_t
    L.jxlhip_parse_metadata.argtypes = [C.c_char_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(ErrorInfo)]
    err = ErrorInfo()
    st = C.c_int32(0)
    n = L.jxlhip_parse_metadata(data, len(data), which, None, 0, C.byref(st), C.byref(err))
    if st.value != 0 or n == 0:
        return DECODER_STATUS[st.value], None, err.errorMessage.decode("ascii", "replace")
    buf = (C.c_uint8 * n)()
    L.jxlhip_parse_metadata(data, len(data), which, buf, n, C.byref(st), C.byref(err))
    return DECODER_STATUS[st.value], bytes(buf), ""


def static_table(name, index, dtype):
    L = lib()
    n = L.jxlhip_static_table(name.encode(), index, None, 0)
    buf = np.empty(n // np.dtype(dtype).itemsize, dtype)
    L.jxlhip_static_table(name.encode(), index, buf.ctypes.data, n)
    return buf


_PLANE_DTYPES = {"lf": np.float32, "lf_quant": np.int32, "cellinfo": np.uint32, "raw_quant": np.uint16, "sharpness": np.uint8,
                 "ytox": np.int8, "ytob": np.int8, "alpha": np.uint8, "inv_sigma": np.float32, "qcoef": np.int32,
                 "xyb_idct": np.float32, "xyb_filtered": np.float32, "noise_rnd": np.float32, "noise": np.float32}


def _last_stage_times(fn_name):
    L = lib()
    fn = getattr(L, fn_name)
    fn.restype = C.c_int32
    fn.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int32]
    names = (C.c_char_p * 32)()
    ms = (C.c_float * 32)()
    k = fn(names, ms, 32)
    return {names[i].decode(): ms[i] for i in range(k)}


def last_load_stage_times():
    """Device time per stage of this thread's last load_image() call (HIP events)."""
    return _last_stage_times("jxlhip_last_load_stage_times")


def last_save_stage_times():
    """Device time per kernel group of this thread's last lossy save_image() call (HIP events)."""
    return _last_stage_times("jxlhip_last_save_stage_times")


def _bgra_surface(bgra):
    bgra = np.asarray(bgra, dtype=np.uint8)
    if bgra.ndim != 3 or bgra.shape[2] != 4:
        raise ValueError("a (h, w, 4) BGRA surface is expected")
    if bgra.strides[2] != 1 or (bgra.shape[1] > 1 and bgra.strides[1] != 4):
        bgra = np.ascontiguousarray(bgra)
    h, w, _ = bgra.shape
    return bgra, w, h, bgra.strides[0] if h > 1 else w * 4


def distance_map(a, b):
    """Cell distances (float32, ceil(h / 8) x ceil(w / 8)) of the BGRA surface b against the original a, by this project's distance
    map (not Butteraugli).  Alpha is ignored."""
    L = lib()
    a, w, h, stride_a = _bgra_surface(a)
    b, wb, hb, stride_b = _bgra_surface(b)
    if (w, h) != (wb, hb):
        raise ValueError("the two pictures differ in size")
    out = np.empty(((h + 7) // 8, (w + 7) // 8), np.float32)
    err = ErrorInfo()
    st = L.jxlhip_distance_map(a.ctypes.data, stride_a, b.ctypes.data, stride_b, w, h, out.ctypes.data, out.size, C.byref(err))
    if st != 0:
        raise JxlError(ENCODER_STATUS[st] if 0 <= st < len(ENCODER_STATUS) else str(st), err.errorMessage.decode("ascii", "replace"))
    return out


def last_save_distances():
    """The closed loop's figures of this thread's last save_image(): dict with `cells` (float32, flat, of the evaluation whose quant
    field was written), `evaluations` (0: the loop did not run), `target`, `cells_over_target_first`, `cells_over_target_emitted`."""
    L = lib()
    ev, first, emitted, target = C.c_int32(), C.c_int32(), C.c_int32(), C.c_float()
    n = L.jxlhip_last_save_distances(None, 0, C.byref(ev), C.byref(target), C.byref(first), C.byref(emitted))
    cells = np.empty(n, np.float32)
    if n:
        L.jxlhip_last_save_distances(cells.ctypes.data, n, None, None, None, None)
    return {"cells": cells, "evaluations": ev.value, "target": target.value, "cells_over_target_first": first.value,
            "cells_over_target_emitted": emitted.value}


def last_save_lossless_info():
    """What the search of this thread's last lossless save_image() chose: dict with `tier` (8 or 9; 0 after a lossy save or an effort
    below 8, and then everything else is 0), `palette_colours` (0: none), `rct_type` (-1: not RGB, or a palette), `predictors` (one per
    coded channel), `leaves`, `clusters`, `fell_back_to_effort7`, `searched_bytes`, `effort7_bytes` (bare codestreams)."""
    info = LosslessInfo()
    lib().jxlhip_last_save_lossless_info(C.byref(info))
    return {"tier": info.tier, "palette_colours": info.palette_colours, "rct_type": info.rct_type,
            "predictors": [info.predictor[c] for c in range(info.num_channels)], "leaves": info.leaves, "clusters": info.clusters,
            "fell_back_to_effort7": bool(info.fell_back_to_effort7), "searched_bytes": info.searched_bytes,
            "effort7_bytes": info.effort7_bytes}


class Decoder:
    """Device-resident batch decoder (jxlhip_* entry points)."""

    def __init__(self, device=-1):
        self._h = None
        self._last_n = self._max_n = 0      # files of the last decode_batch call / of the largest one (finish's status buffer)
        self.last_error = ""
        self._L = lib()
        err = ErrorInfo()
        self._h = self._L.jxlhip_decoder_create(device, C.byref(err))
        if not self._h:
            raise JxlError("DecoderCreate", err.errorMessage.decode("ascii", "replace"))

    def close(self):
        if self._h:
            self._L.jxlhip_decoder_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def set_option(self, name, value):
        """Returns 1 when the option was set, 0 for an unknown name or a refused value (the previous value is kept).  "downscale": 1
        (full size) or 8 - every image of the next batches is decoded at 1:8, see decode_batch."""
        return self._L.jxlhip_set_option(self._h, name.encode(), int(value))

    def decode_batch(self, files, dev_out_ptrs, dev_data_ptrs=None, stream=None, synchronize=True, raise_on_error=True):
        """files: list of bytes; dev_out_ptrs: device pointers (ints); dev_data_ptrs: device pointers of resident file bytes.

        Each output buffer receives width x height pixels, tight rows, of num_channels samples of bytes_per_sample bytes, with
        (width, height) as `peek` reports them - or, after set_option("downscale", 8), reduced_size(width, height, 8) of them: the
        buffer must hold at least rw * rh * num_channels * bytes_per_sample bytes for (rw, rh) = reduced_size(...).  At 1:8 layered
        files, files with patches and band decodes are refused per image (DecodeError); the other images of the batch decode."""
        n = len(files)
        hd = (C.c_char_p * n)(*files)
        sz = (C.c_size_t * n)(*[len(f) for f in files])
        dd = (C.c_void_p * n)(*(dev_data_ptrs or [None] * n))
        do = (C.c_void_p * n)(*dev_out_ptrs)
        st = (C.c_int32 * n)()
        err = ErrorInfo()
        self._keep = (hd, sz, dd, do)
        self._last_n, self._max_n = n, max(n, self._max_n)   # (finish: a batch that failed to submit leaves the one before it the most recent)
        r = self._L.jxlhip_decode_batch(self._h, n, hd, sz, dd, do, stream, 1 if synchronize else 0, st, C.byref(err))
        self.last_error = err.errorMessage.decode("ascii", "replace")
        if r != 0 and raise_on_error:
            raise FormatError(DECODER_STATUS[r] if 0 <= r < len(DECODER_STATUS) else str(r), self.last_error)
        return list(st)

    def finish(self, raise_on_error=True):
        """Waits for every asynchronous batch, oldest first.  Returns (status name, per-file statuses of the most recent batch), the
        message in last_error.  The status is the most recent batch's or, that one being Ok, that of an older batch whose failure has
        not been reported yet ("an earlier asynchronous batch failed: ...", reported once); with raise_on_error it raises FormatError
        instead of returning a status that is not Ok.  (The list has one entry per file of the last decode_batch call; after a call
        that failed before it submitted anything, the batch before it is the most recent one and the list's length is not its.)"""
        n = self._last_n
        st = (C.c_int32 * max(self._max_n, 1))()
        err = ErrorInfo()
        r = self._L.jxlhip_finish(self._h, st if n else None, C.byref(err))
        self.last_error = err.errorMessage.decode("ascii", "replace")
        name = DECODER_STATUS[r] if 0 <= r < len(DECODER_STATUS) else str(r)
        if r != 0 and raise_on_error:
            raise FormatError(name, self.last_error)
        return name, list(st[:n])

    def read_plane(self, index, name, channel=0):
        n = self._L.jxlhip_read_plane(self._h, index, name.encode(), channel, None, 0)
        if n == 0:
            raise KeyError(name)
        buf = np.empty(n // np.dtype(_PLANE_DTYPES[name]).itemsize, _PLANE_DTYPES[name])
        self._L.jxlhip_read_plane(self._h, index, name.encode(), channel, buf.ctypes.data, n)
        return buf

    def stage_totals(self, reset=False):
        """({stage: cumulative ms}, batches) over every batch finished since the last reset."""
        names = (C.c_char_p * 16)()
        ms = (C.c_float * 16)()
        nb = C.c_int32()
        k = self._L.jxlhip_stage_totals(self._h, names, ms, 16, C.byref(nb), 1 if reset else 0)
        return {names[i].decode(): ms[i] for i in range(k)}, nb.value

    def stage_times(self):
        names = (C.c_char_p * 16)()
        ms = (C.c_float * 16)()
        k = self._L.jxlhip_stage_times(self._h, names, ms, 16)
        return {names[i].decode(): ms[i] for i in range(k)}


class EncodeItem:
    """One image of Encoder.encode_batch: pixels in DEVICE memory and how to encode them.

    ptr: device pointer (int) of interleaved samples, Gray | Gray,A | R,G,B | R,G,B,A; dtype: numpy dtype of a sample (uint8, uint16,
    float16, float32); stride_bytes: bytes from one row to the next (default: tight rows); bits: of integer samples (default 8 / 16).
    The other arguments are save_pixels' own (cfl: True / False or a JxlHipLossyOptions).  `from_tensor` takes a torch tensor (h, w[, c]) on the GPU, rows may be strided."""

    def __init__(self, ptr, width, height, channels, dtype, stride_bytes=None, bits=None, colour="Srgb", distance=1.0, effort=7,
                 lossless=False, exif=None, xmp=None, icc=None, keep=None, cfl=False):
        dtype = np.dtype(dtype)
        if dtype not in _SAMPLE_TYPES:
            raise ValueError("samples are uint8, uint16, float16 or float32")
        self.ptr, self.width, self.height, self.channels, self.dtype = ptr, int(width), int(height), int(channels), dtype
        self.stride_bytes = int(stride_bytes) if stride_bytes is not None else self.width * self.channels * dtype.itemsize
        self.bits = ({1: 8, 2: 16}[dtype.itemsize] if dtype.kind == "u" else 0) if bits is None else int(bits)
        self.colour, self.distance, self.effort, self.lossless = colour, float(distance), int(effort), bool(lossless)
        self.exif, self.xmp, self.icc = exif, xmp, icc
        self.cfl = cfl
        self.keep = keep   # whatever owns the device memory

    @classmethod
    def from_tensor(cls, t, **kw):
        if t.dim() == 2:
            t = t.unsqueeze(2)
        h, w, c = t.shape
        item = t.element_size()
        if t.stride(2) != 1 or (w > 1 and t.stride(1) != c) or (h > 1 and t.stride(0) < w * c):
            t = t.contiguous()
        dtype = {"torch.uint8": np.uint8, "torch.uint16": np.uint16, "torch.int16": np.uint16, "torch.float16": np.float16,
                 "torch.float32": np.float32}[str(t.dtype)]
        return cls(t.data_ptr(), w, h, c, dtype, stride_bytes=t.stride(0) * item if h > 1 else w * c * item, keep=t, **kw)


class Encoder:
    """Device-resident batch encoder (jxlhip_encoder_* / jxlhip_encode_batch): many images already in HBM, encoded in one call.
    The file of each image is byte for byte what save_pixels writes for the same pixels and arguments."""

    def __init__(self, device=-1):
        self._h = None
        self._L = lib()
        err = ErrorInfo()
        self._h = self._L.jxlhip_encoder_create(device, C.byref(err))
        if not self._h:
            raise JxlError("EncoderCreate", err.errorMessage.decode("ascii", "replace"))
        self.last_error = ""
        self.last_statuses = []

    def close(self):
        if self._h:
            self._L.jxlhip_encoder_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def encode_batch(self, items, raise_on_error=True, lossy_call=None):
        """items: list of EncodeItem.  Returns one bytes object per image (None for an image that was refused or failed; its status
        name is in last_statuses[i], the first message in last_error).  Synchronous.  With raise_on_error the first status that is not
        Ok raises JxlError.  lossy_call: None - jxlhip_encode_batch_lossy when an item sets cfl, jxlhip_encode_batch otherwise; True -
        jxlhip_encode_batch_lossy with every item's options; "null" - jxlhip_encode_batch_lossy without options (NULL)."""
        n = len(items)
        px = (JxlHipPixels * max(n, 1))()
        opt = (EncoderOptions * max(n, 1))()
        mds = (C.POINTER(EncoderImageMetadata) * max(n, 1))()
        keep = []
        for i, it in enumerate(items):
            px[i] = JxlHipPixels(it.ptr, it.width, it.height, it.stride_bytes, it.channels, _SAMPLE_TYPES[it.dtype], it.bits,
                                 KNOWN_PROFILE.index(it.colour))
            opt[i] = EncoderOptions(it.distance, it.effort, it.lossless)
            if it.exif or it.xmp or it.icc:
                bufs = [np.frombuffer(b, np.uint8) if b else None for b in (it.exif, it.icc, it.xmp)]
                md = EncoderImageMetadata(*sum(([k.ctypes.data if k is not None else None, len(k) if k is not None else 0] for k in bufs), []))
                keep.append((bufs, md))
                mds[i] = C.pointer(md)
        st = (C.c_int32 * max(n, 1))()
        err = ErrorInfo()
        if lossy_call is None:
            lossy_call = any(isinstance(it.cfl, JxlHipLossyOptions) or it.cfl for it in items)
        if lossy_call:
            lossy = None if lossy_call == "null" else (JxlHipLossyOptions * max(n, 1))(*[_lossy_options(it.cfl) for it in items])
            r = self._L.jxlhip_encode_batch_lossy(self._h, n, px, opt, lossy, mds, st, C.byref(err))
        else:
            r = self._L.jxlhip_encode_batch(self._h, n, px, opt, mds, st, C.byref(err))
        self.last_error = err.errorMessage.decode("ascii", "replace")
        self.last_statuses = [ENCODER_STATUS[st[i]] if 0 <= st[i] < len(ENCODER_STATUS) else str(st[i]) for i in range(n)]
        if r != 0 and raise_on_error:
            raise JxlError(ENCODER_STATUS[r] if 0 <= r < len(ENCODER_STATUS) else str(r), self.last_error)
        out = []
        for i in range(n):
            p, size = C.c_void_p(), C.c_size_t()
            out.append(C.string_at(p.value, size.value) if self._L.jxlhip_encoder_result(self._h, i, C.byref(p), C.byref(size)) else None)
        return out

    def encode_animation(self, frames, durations, tps=(100, 1), loops=0, key_interval=0, chunk_frames=0, distance=1.0, effort=7,
                         lossless=False, colour=None, bits=None, exif=None, xmp=None, max_rects=1, merge_pixels=4096, tolerance=0.0):
        """jxlhip_encode_animation_changes: the frames as ONE animated file (bytes).  frames: a list of EncodeItem / GPU tensors (h, w[, c]), or
        one GPU tensor [n, h, w, c]; all of one size, channel count and sample type.  durations: ticks per frame (>= 1), one per frame
        or one number for all; tps: ticks per second as (numerator, denominator); loops: 0 = endless.  Frame 0 - and with
        key_interval >= 1 every key_interval-th frame - is written whole, every other frame as the rectangle that changed against its
        predecessor (lossy: grown to multiples of 8 pixels), a frame that changed nothing as one pixel; last_animation_rects has
        them.  max_rects >= 2 (up to 16): what changed is measured per 64 x 64 tile and such a frame is written as up to max_rects
        disjoint rectangles - the groups of touching changed tiles, merged while there are too many or while merging two codes at
        most merge_pixels pixels more - each a frame of the codestream, all but the last without a duration;
        last_animation_frame_rects has them, last_animation_tiles(pair) the tile map.  max_rects = 1 is jxlhip_encode_animation byte
        for byte (merge_pixels plays no part).  tolerance > 0: a sample counts as changed only when it moved by more than the tolerance
        (integers: by more than floor(tolerance); floats: equal bits, or both finite and |a - b| <= tolerance in binary32, are
        unchanged) - every sample of every channel, alpha included - and a frame is compared not with its predecessor but with a
        reference canvas on the device that holds the source of what a decoder shows: frame 0, then each written rectangle (the 1 x 1
        of an unchanged frame and the lossy growth to the 8-pixel grid included) copied in.  So no displayed sample is further than
        the tolerance from its source, before coding error, in any frame; with lossless=True the coded rectangles are exact and the
        rest is within the tolerance.  last_animation_tiles(pair) then has a map for every pair whatever max_rects is.  tolerance = 0
        (the default) is the bit rule against the predecessor, byte for byte the file without the argument.  chunk_frames: codestream frames that go through the encoder at a time (0: by its workspace budget; the bytes do not depend on it).
        distance, effort, lossless hold for every frame; colour and bits default to those of the first EncodeItem (tensors: "Srgb",
        8 / 16 bits).  Raises JxlError where the call is refused or fails; the encoder stays usable."""
        if hasattr(frames, "dim") and not isinstance(frames, (list, tuple)):
            frames = [frames[k] for k in range(frames.shape[0])]
        items = [f if isinstance(f, EncodeItem) else EncodeItem.from_tensor(f) for f in frames]
        n = len(items)
        if not hasattr(durations, "__len__"):
            durations = [durations] * n
        if len(durations) != n:
            raise ValueError("one duration per frame is expected")
        px = (JxlHipPixels * max(n, 1))()
        for i, it in enumerate(items):
            px[i] = JxlHipPixels(it.ptr, it.width, it.height, it.stride_bytes, it.channels, _SAMPLE_TYPES[it.dtype],
                                 it.bits if bits is None else int(bits), KNOWN_PROFILE.index(it.colour if colour is None else colour))
        dur = (C.c_uint32 * max(n, 1))(*[int(d) for d in durations])
        opt = EncoderOptions(float(distance), int(effort), bool(lossless))
        ao = AnimationOptions(int(tps[0]), int(tps[1]), int(loops), int(key_interval), int(chunk_frames))
        bufs = [np.frombuffer(b, np.uint8) if b else None for b in (exif, None, xmp)]
        md = EncoderImageMetadata(*sum(([k.ctypes.data if k is not None else None, len(k) if k is not None else 0] for k in bufs), []))
        err = ErrorInfo()
        ro = AnimationRectOptions(int(max_rects), int(merge_pixels))
        co = AnimationChangeOptions(float(tolerance))
        r = self._L.jxlhip_encode_animation_changes(self._h, n, px, dur, C.byref(opt), C.byref(ao), C.byref(ro), C.byref(co), C.byref(md), C.byref(err))
        self.last_error = err.errorMessage.decode("ascii", "replace")
        if r != 0:
            raise JxlError(ENCODER_STATUS[r] if 0 <= r < len(ENCODER_STATUS) else str(r), self.last_error)
        p, size = C.c_void_p(), C.c_size_t()
        if not self._L.jxlhip_encoder_result(self._h, 0, C.byref(p), C.byref(size)):
            raise JxlError("EncodeError", "the encoder holds no result")
        return C.string_at(p.value, size.value)

    @property
    def last_animation_rects(self):
        """[(x, y, width, height)] per frame of the last encode_animation that got as far as measuring what changed."""
        n = self._L.jxlhip_encoder_animation_rects(self._h, None, 0)
        buf = (C.c_int32 * (4 * max(n, 1)))()
        self._L.jxlhip_encoder_animation_rects(self._h, buf, n)
        return [tuple(buf[4 * k:4 * k + 4]) for k in range(n)]

    @property
    def last_animation_frame_rects(self):
        """[(input frame, x, y, width, height)] per codestream frame of the last encode_animation, in file order: a frame written as m
        rectangles appears m times."""
        n = self._L.jxlhip_encoder_animation_frame_rects(self._h, None, 0)
        buf = (C.c_int32 * (5 * max(n, 1)))()
        self._L.jxlhip_encoder_animation_frame_rects(self._h, buf, n)
        return [tuple(buf[5 * c:5 * c + 5]) for c in range(n)]

    def last_animation_tiles(self, pair):
        """The tile map of frames `pair` and `pair + 1` of the last encode_animation with max_rects >= 2: a (tiles down, tiles across,
        4) uint8 array of x0, y0, x1, y1 - the inclusive box, relative to the tile, of the changed pixels in each 64 x 64 tile - with
        255 everywhere for a tile in which nothing changed.  With a tolerance > 0: the map of frame `pair + 1` against the reference
        canvas as it stood before that frame, for every pair whatever max_rects was, key frames included.  Raises ValueError where
        there is no such pair."""
        n = self._L.jxlhip_encoder_animation_tiles(self._h, int(pair), None, 0)
        if n == 0:
            raise ValueError("no tile map for pair %d: the last animation has no such pair or was encoded with max_rects = 1 and no tolerance" % pair)
        buf = np.zeros(n, np.uint32)
        self._L.jxlhip_encoder_animation_tiles(self._h, int(pair), buf.ctypes.data_as(C.POINTER(C.c_uint32)), n)
        rects = self.last_animation_rects
        w, h = rects[0][2], rects[0][3]                       # frame 0 is the canvas
        return buf.view(np.uint8).reshape((h + 63) // 64, (w + 63) // 64, 4)

    def stage_times(self):
        """{stage: ms} of the last batch: device time per kernel group (stages on different streams overlap), then the host's stages
        ("host: ...") on the host clock."""
        names = (C.c_char_p * 48)()
        ms = (C.c_float * 48)()
        k = self._L.jxlhip_encoder_stage_times(self._h, names, ms, 48)
        return {names[i].decode(): ms[i] for i in range(k)}


class Animation:
    """Every displayed image of a file, in file order, decoded to device memory (jxlhip_animation_*).  A context manager:

        with api.Animation(data) as a:
            a.info.num_displayed, a.frames[0].duration
            t = a.next(4)          # torch tensor [n, h, w, c] on the GPU, n <= 4 (0 at the end)
            a.rewind()
            every = a.read_all()   # numpy [num_displayed, h, w, c]
            a.entry_points         # [0, 8, 16, ...]: the images a decode can start at
            a.seek(20); a.next(1)  # image 20, decoded from image 16 on; images 16 .. 19 are not stored
            one = a.frame(20)      # the same
            a.rewind()
            small = a.thumbnails(step=4)   # images 0, 4, 8, ... at 1:8, [n, ceil(h / 8), ceil(w / 8), c]

    Decoding is sequential from an entry point (the state between two images is the reference slots): image 0, and every image in
    front of which no slot is alive - an encoder's key frames are such.  A file without an animation header has one displayed image,
    the one load_image delivers.  Raises FormatError where the file is refused."""

    def __init__(self, data, device=-1):
        self._h = None
        self._L = lib()
        self.info = AnimationInfo()
        self._device, self._pos = device, 0
        err = ErrorInfo()
        self._h = self._L.jxlhip_animation_open(device, data, len(data), C.byref(self.info), C.byref(err))
        if not self._h:
            raise FormatError("DecodeError", err.errorMessage.decode("ascii", "replace"))
        self.frames = []
        for j in range(self.info.num_displayed):
            fr = AnimationFrame()
            self._L.jxlhip_animation_frame(self._h, j, C.byref(fr))
            fr.name_bytes = fr.name[:fr.name_length] if fr.name_length else b""
            self.frames.append(fr)
        i = self.info
        if i.float_samples:
            self.dtype = np.float16 if i.bytes_per_sample == 2 else np.float32
        else:
            self.dtype = np.uint16 if i.bytes_per_sample == 2 else np.uint8

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self._h:
            self._L.jxlhip_animation_close(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def set_option(self, name, value):
        """"chunk_frames": 0 (chunks by the decoder's limits) or n >= 1 (at most n codestream frames per chunk; same output), and the
        decoder's "lane_stride", "no_direct", "mod_lanes64", "no_stream_pairs", "no_lf_pipeline".  Returns 1 when the option was set,
        0 for any other name."""
        return self._L.jxlhip_animation_set_option(self._h, name.encode(), int(value))

    def rewind(self):
        self._L.jxlhip_animation_rewind(self._h)
        self._pos = 0

    @property
    def entry_points(self):
        """The displayed images at which decoding can start (ascending, 0 first): seek() resumes at the nearest one in front."""
        n = self._L.jxlhip_animation_entry_points(self._h, None, 0)
        buf = (C.c_int32 * max(1, n))()
        self._L.jxlhip_animation_entry_points(self._h, buf, n)
        return list(buf[:n])

    @property
    def position(self):
        """(codestream frame the next chunk starts at, displayed image that next() delivers first)."""
        f, j = C.c_int32(0), C.c_int32(0)
        self._L.jxlhip_animation_position(self._h, C.byref(f), C.byref(j))
        return f.value, j.value

    def seek(self, j):
        """next() delivers displayed image j after it (j == num_displayed: the end).  Lazy: nothing is decoded by the call, and the images
        between the entry point and j are never stored.  ValueError for a j outside the file."""
        err = ErrorInfo()
        st = self._L.jxlhip_animation_seek(self._h, int(j), C.byref(err))
        self.last_error = err.errorMessage.decode("ascii", "replace")
        if st != 0:
            name = DECODER_STATUS[st] if 0 <= st < len(DECODER_STATUS) else str(st)
            if name == "InvalidParameter":
                raise ValueError(self.last_error)
            raise FormatError(name, self.last_error)
        self._pos = int(j)

    def frame(self, j):
        """Displayed image j as a torch tensor [h, w, c] on the device: seek(j), then next(1)[0]."""
        self.seek(j)
        t = self.next(1)
        if t.shape[0] != 1:
            raise ValueError("displayed image %d: the file has %d" % (j, self.info.num_displayed))
        return t[0]

    def thumbnails(self, count=None, step=1):
        """Displayed images p, p + step, ... (p: the position) at 1:8 as a torch tensor [n, rh, rw, c] on the device, (rw, rh) =
        reduced_size(width, height, 8): each sample the mean of an 8 x 8 cell of what next() stores.  count None: every selected image
        that is left.  The images in between are decoded, not stored.  16-bit integers arrive as torch.int16 holding the same bits."""
        import torch
        i = self.info
        if step < 1:
            raise ValueError("step %d: step >= 1" % step)
        left = max(0, (i.num_displayed - self._pos + step - 1) // step)
        want = left if count is None else max(0, min(int(count), left))
        rw, rh = reduced_size(i.width, i.height, 8)
        tdt = {np.uint8: torch.uint8, np.uint16: torch.int16, np.float16: torch.float16, np.float32: torch.float32}[self.dtype]
        dev = torch.device("cuda", self._device) if self._device >= 0 else torch.device("cuda")
        out = torch.empty((want, rh, rw, i.num_channels), dtype=tdt, device=dev)
        torch.cuda.synchronize()
        n = C.c_int32(0)
        err = ErrorInfo()
        st = self._L.jxlhip_animation_next_reduced(self._h, want, int(step), out.data_ptr() if want else None, out.numel() * out.element_size(),
                                                   C.byref(n), C.byref(err))
        self.last_error = err.errorMessage.decode("ascii", "replace")
        self._pos = self.position[1]
        if st != 0:
            raise FormatError(DECODER_STATUS[st] if 0 <= st < len(DECODER_STATUS) else str(st), self.last_error)
        return out[:n.value]

    def read_thumbnails(self, step=1):
        """Rewinds and returns the 1:8 images 0, step, 2 step, ... as one numpy array [n, rh, rw, c] of the file's sample type."""
        self.rewind()
        a = self.thumbnails(None, step).cpu().numpy()
        return a.view(np.uint16) if self.dtype == np.uint16 else a

    def next(self, count=1):
        """The next `count` displayed images as a torch tensor [n, h, w, c] on the device (n < count at the end of the file, 0 behind
        it).  16-bit integer samples arrive as torch.int16 holding the same bits (read_all() hands them out as numpy uint16)."""
        import torch
        i = self.info
        tdt = {np.uint8: torch.uint8, np.uint16: torch.int16, np.float16: torch.float16, np.float32: torch.float32}[self.dtype]
        want = max(0, min(count, i.num_displayed - self._pos))   # (nothing is allocated for images behind the end of the file)
        dev = torch.device("cuda", self._device) if self._device >= 0 else torch.device("cuda")
        out = torch.empty((want, i.height, i.width, i.num_channels), dtype=tdt, device=dev)
        torch.cuda.synchronize()
        n = C.c_int32(0)
        err = ErrorInfo()
        st = self._L.jxlhip_animation_next(self._h, want, out.data_ptr() if want else None, out.numel() * out.element_size(), C.byref(n), C.byref(err))
        self.last_error = err.errorMessage.decode("ascii", "replace")
        if st != 0:
            raise FormatError(DECODER_STATUS[st] if 0 <= st < len(DECODER_STATUS) else str(st), self.last_error)
        self._pos += n.value
        return out[:n.value]

    def read_all(self):
        """Rewinds and returns every displayed image as one numpy array [num_displayed, h, w, c] of the file's sample type."""
        self.rewind()
        t = self.next(self.info.num_displayed)
        a = t.cpu().numpy()
        return a.view(np.uint16) if self.dtype == np.uint16 else a

    def decoder_stage_totals(self, reset=False):
        """({stage: cumulative ms}, chunks) of the animation's decoder over every chunk since the last reset (HIP events), as
        Decoder.stage_totals: a call of next() runs one batch per chunk."""
        L = self._L
        names = (C.c_char_p * 16)()
        ms = (C.c_float * 16)()
        nb = C.c_int32()
        k = L.jxlhip_stage_totals(L.jxlhip_animation_decoder(self._h), names, ms, 16, C.byref(nb), 1 if reset else 0)
        return {names[i].decode(): ms[i] for i in range(k)}, nb.value
