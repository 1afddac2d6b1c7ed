"""ctypes binding of the CPU oracle (oracle/_build/libjxo.so) — test infrastructure only."""
import ctypes as C
import os
import subprocess
import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(_ROOT, "oracle", "_build", "libjxo.so")


class EncodeParams(C.Structure):
    _fields_ = [("distance", C.c_float), ("lossless", C.c_int32), ("effort", C.c_int32), ("strategy_mode", C.c_int32),
                ("fixed_strategy", C.c_int32), ("seed", C.c_uint32), ("epf_iters", C.c_int32), ("gaborish", C.c_int32),
                ("container", C.c_int32), ("adaptive_lf_smoothing", C.c_int32), ("lossless_predictor", C.c_int32),
                ("lossless_squeeze", C.c_int32), ("lossless_tree", C.c_int32), ("num_threads", C.c_int32), ("bits", C.c_int32), ("orientation", C.c_int32), ("float_samples", C.c_int32), ("colour", C.c_int32)]


class SideInfo(C.Structure):
    """oracle/jxo_codec.h: SideInfo (the side information of a lossy frame that the writer can vary), field for field."""
    _fields_ = [("cfl_mode", C.c_int32), ("sharp_mode", C.c_int32), ("sharp_value", C.c_int32), ("seed", C.c_uint32), ("refuse", C.c_int32),
                ("custom_cfl", C.c_int32), ("color_factor", C.c_uint32), ("base_x", C.c_float), ("base_b", C.c_float),
                ("ytox_lf", C.c_int32), ("ytob_lf", C.c_int32), ("custom_lf_factors", C.c_int32), ("lf_factor", C.c_float * 3),
                ("x_qm_scale", C.c_int32), ("b_qm_scale", C.c_int32), ("custom_gab", C.c_int32), ("gab_w1", C.c_float * 3),
                ("gab_w2", C.c_float * 3), ("custom_sharp_lut", C.c_int32), ("sharp_lut", C.c_float * 8), ("custom_epf_weights", C.c_int32),
                ("epf_channel_scale", C.c_float * 3), ("custom_epf_sigma", C.c_int32), ("epf_quant_mul", C.c_float),
                ("epf_pass0_sigma_scale", C.c_float), ("epf_pass2_sigma_scale", C.c_float), ("epf_border_sad_mul", C.c_float),
                ("custom_transform", C.c_int32), ("quant_bias", C.c_float * 4)]


_CFL_MODES = {"zero": 0, "fitted": 1, "formula": 2}


def make_side_info(cfl=None, sharpness=None, seed=0, refuse=None, cfl_params=None, lf_factors=None, qm_scales=None, gaborish_weights=None,
                   sharp_lut=None, epf_channel_scale=None, epf_sigma=None, quant_biases=None):
    """The keyword arguments of encode(side_info=dict(...)):
    cfl: "fitted" / "formula"; sharpness: "formula" or a constant 0..7 (one token per cell; None keeps the stream's leaf-offset 4);
    seed: of the two formulas; refuse: "sharpness" / "cfl" (one value out of range, for refusal tests);
    cfl_params: (color_factor, base_correlation_x, base_correlation_b, ytox_lf, ytob_lf); lf_factors: three stored values (128 x step);
    qm_scales: (x_qm_scale, b_qm_scale); gaborish_weights: ((w1, w2) for X, Y, B); sharp_lut: eight values;
    epf_channel_scale: three values; epf_sigma: (quant_mul, pass0_sigma_scale, pass2_sigma_scale, border_sad_mul);
    quant_biases: four values, written in a custom transform-data bundle whose opsin values are the defaults as F16 rounds them."""
    s = SideInfo()
    s.cfl_mode = _CFL_MODES[cfl or "zero"]
    s.seed = seed
    if sharpness == "formula":
        s.sharp_mode = 1
    elif sharpness is not None:
        s.sharp_mode, s.sharp_value = 2, int(sharpness)
    s.refuse = {None: 0, "sharpness": 1, "cfl": 2}[refuse]
    s.color_factor, s.base_x, s.base_b = 84, 0.0, 1.0
    if cfl_params is not None:
        s.custom_cfl = 1
        s.color_factor, s.base_x, s.base_b, s.ytox_lf, s.ytob_lf = cfl_params
    if lf_factors is not None:
        s.custom_lf_factors = 1
        s.lf_factor[:] = lf_factors
    s.x_qm_scale, s.b_qm_scale = qm_scales if qm_scales is not None else (-1, -1)
    if gaborish_weights is not None:
        s.custom_gab = 1
        s.gab_w1[:] = [w[0] for w in gaborish_weights]
        s.gab_w2[:] = [w[1] for w in gaborish_weights]
    if sharp_lut is not None:
        s.custom_sharp_lut = 1
        s.sharp_lut[:] = sharp_lut
    if epf_channel_scale is not None:
        s.custom_epf_weights = 1
        s.epf_channel_scale[:] = epf_channel_scale
    if epf_sigma is not None:
        s.custom_epf_sigma = 1
        s.epf_quant_mul, s.epf_pass0_sigma_scale, s.epf_pass2_sigma_scale, s.epf_border_sad_mul = epf_sigma
    if quant_biases is not None:
        s.custom_transform = 1
        s.quant_bias[:] = quant_biases
    return s


def build():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(_ROOT, "oracle")])


def build_native():
    """-O3 -march=native build for the machine this runs on (bench.py's cpu_baseline leg; the default build is portable because it
    travels from the build container to the GPU box).  Returns the path of the library."""
    # keyed by the CPU's feature flags: a build made elsewhere (e.g. in the container the repo was snapshotted from) is never reused
    import hashlib
    try:
        flags = [l for l in open("/proc/cpuinfo") if l.startswith("flags")][0]
    except Exception:
        flags = "unknown"
    out = os.path.join("_build", "native-" + hashlib.sha1(flags.encode()).hexdigest()[:10])
    subprocess.check_call(["make", "-s", "-j16", "-C", os.path.join(_ROOT, "oracle"), "BUILD=" + out,
                           "CXXFLAGS=-O3 -march=native -std=c++17 -fPIC -pthread"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.join(_ROOT, "oracle", out, "libjxo.so")


def use(path):
    """Binds a different build of the oracle library (before or after the first call)."""
    global _lib, _SO
    _SO = path
    _lib = None


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            build()
        L = C.CDLL(_SO)
        L.jxo_last_error.restype = C.c_char_p
        L.jxo_decode.restype = C.c_void_p
        L.jxo_decode.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int]
        L.jxo_image_free.argtypes = [C.c_void_p]
        L.jxo_image_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_int32)] * 5
        L.jxo_image_pixels.restype = C.POINTER(C.c_uint8)
        L.jxo_image_pixels.argtypes = [C.c_void_p]
        L.jxo_image_epf_iters.argtypes = [C.c_void_p]
        L.jxo_image_exif.restype = C.c_size_t
        L.jxo_image_exif.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint8))]
        L.jxo_image_xml.restype = C.c_size_t
        L.jxo_image_xml.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint8))]
        L.jxo_image_plane.restype = C.c_size_t
        L.jxo_image_plane.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]
        L.jxo_encode.restype = C.c_void_p
        L.jxo_encode.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.POINTER(EncodeParams), C.c_char_p, C.c_size_t,
                                 C.c_char_p, C.c_size_t]
        L.jxo_bytes_data.restype = C.POINTER(C.c_uint8)
        L.jxo_bytes_data.argtypes = [C.c_void_p]
        L.jxo_bytes_size.restype = C.c_size_t
        L.jxo_bytes_size.argtypes = [C.c_void_p]
        L.jxo_bytes_free.argtypes = [C.c_void_p]
        _lib = L
    return _lib


class OracleError(RuntimeError):
    pass


def flatten_transforms(transforms):
    """encode(transforms=...) as the flat ints of oracle/jxo_codec.h: EncodeParams::transforms."""
    def squeezes(lst):
        out = [len(lst)]
        for hor, in_place, begin_c, num_c in lst:
            out += [int(hor), int(in_place), begin_c, num_c]
        return out
    flat = []
    for t in transforms:
        if t[0] == "rct":
            flat += [0, t[1], t[2]]
        elif t[0] == "palette":
            flat += [1, t[1], t[2]]
        elif t[0] == "squeeze":
            flat += [2] + squeezes(t[1])
        elif t[0] == "declare":
            flat += [3, t[1]] + (squeezes(t[2]) if t[1] == 2 else list(t[2:]))
        else:
            raise OracleError("transforms: unknown entry %r" % (t,))
    return flat


_DEFAULT_DISTANCES = (0, 1)


def flatten_entropy(e):
    """encode(entropy=...) as the flat ints of oracle/jxo_api.cc: jxo_set_next_entropy.  Keys:
    cfgs: [(split, msb, lsb), ...], given to each code's clusters by cluster index, round-robin (clusters are found on default tokens);
    lz: dict(min_symbol, min_length, len_cfg, max_len, distances, general_max, overshoot, zero_start) - implies lz77.  distances is a
      collection of special indices 0..119 and / or "general" (plain distances 1..general_max, default 40); the finder takes the longest
      match, ties to the lowest index, special before general.  On streams without a distance multiplier (HF coefficients) the special
      indices mean "one back".  Without `distances` the writer keeps its own finder (one back, one row back);
    hist: "flat", ("shift", s) or "rle"; ctx_map_mtf: bool;
    bad_cfg: (split, msb, lsb) written as cluster 0's configuration whatever the tokens use; bad_hist: "shift14" / "rle_after_omit"
      (refusal tests: the streams do not decode)."""
    unknown = set(e) - {"cfgs", "lz", "hist", "ctx_map_mtf", "bad_cfg", "bad_hist"}
    if unknown:
        raise OracleError("entropy: unknown keys %s" % sorted(unknown))
    flat = [len(e.get("cfgs", ()))]
    for c in e.get("cfgs", ()):
        flat += [int(v) for v in c]
    lz = e.get("lz")
    unknown = set(lz or ()) - {"min_symbol", "min_length", "len_cfg", "max_len", "distances", "general_max", "overshoot", "zero_start"}
    if unknown:
        raise OracleError("entropy: unknown lz keys %s" % sorted(unknown))
    lz = lz or {}
    dist = lz.get("distances")
    special = sorted(d for d in (dist if dist is not None else _DEFAULT_DISTANCES) if d != "general")
    flat += [int(e.get("lz") is not None), lz.get("min_symbol", 224), lz.get("min_length", 3), lz.get("max_len", 200)]
    flat += list(lz.get("len_cfg", (4, 2, 0)))
    flat += [int(dist is not None), len(special)] + special
    flat += [int(dist is not None and "general" in dist), lz.get("general_max", 40), int(lz.get("overshoot", False)), int(lz.get("zero_start", False))]
    hist = e.get("hist")
    if hist is None:
        flat += [0, 13]
    elif hist == "flat":
        flat += [1, 13]
    elif hist == "rle":
        flat += [3, 13]
    elif isinstance(hist, tuple) and hist[0] == "shift":
        flat += [2, int(hist[1])]
    else:
        raise OracleError("entropy: unknown histogram form %r" % (hist,))
    flat += [int(e.get("ctx_map_mtf", False))]
    flat += [int("bad_cfg" in e)] + list(e.get("bad_cfg", (0, 0, 0))) + [{None: 0, "shift14": 1, "rle_after_omit": 2}[e.get("bad_hist")]]
    return flat


def special_distances():
    """The oracle reader's table of special LZ77 distances: 120 (dx, dy) pairs by index."""
    L = lib()
    L.jxo_special_distance.argtypes = [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    out = []
    for i in range(120):
        dx, dy = C.c_int32(), C.c_int32()
        L.jxo_special_distance(i, C.byref(dx), C.byref(dy))
        out.append((dx.value, dy.value))
    return out


def entropy_census():
    """What the last encode(entropy=...) wrote.  "codes": one dict per top-level code in the order written - contexts, log_alpha,
    prefix, lz77, cfgs (per cluster), special (copies per special index), general (plain-distance copies; general_min / general_max their
    smallest and largest distance as coded, general_small[d] the count of distance d = 1..8), overlapping (distance < length), clamped,
    zero_start, longest_copy, max_tail_bits (the most extra bits read for one value), max_dist_tail_bits (for one distance), the
    histogram forms (hist_simple / hist_flat / hist_flat_not_pow2 / hist_shift {s: n} / hist_rle / rle_to_end / hist_full), mtf_maps and
    mtf_largest.  The same keys at the top level hold the sums (max_*, longest_copy, general_max, mtf_largest: the largest) over the codes."""
    import json
    L = lib()
    L.jxo_entropy_census.restype = C.c_size_t
    L.jxo_entropy_census.argtypes = [C.c_char_p, C.c_size_t]
    n = L.jxo_entropy_census(None, 0)
    buf = C.create_string_buffer(n + 1)
    L.jxo_entropy_census(buf, n)
    cen = json.loads(buf.raw[:n].decode())
    codes = cen["codes"]
    for key in ("general", "overlapping", "clamped", "zero_start", "hist_simple", "hist_flat", "hist_flat_not_pow2", "hist_rle", "rle_to_end",
                "hist_full", "mtf_maps"):
        cen[key] = sum(c[key] for c in codes)
    for key in ("longest_copy", "max_tail_bits", "max_dist_tail_bits", "general_max", "mtf_largest"):
        cen[key] = max([c[key] for c in codes] or [0])
    cen["general_min"] = min([c["general_min"] for c in codes if c["general"]] or [0])
    cen["special"] = [sum(c["special"][k] for c in codes) for k in range(120)]
    cen["general_small"] = [sum(c["general_small"][k] for c in codes) for k in range(9)]
    cen["hist_shift"] = {}
    for c in codes:
        for s, v in c["hist_shift"].items():
            cen["hist_shift"][int(s)] = cen["hist_shift"].get(int(s), 0) + v
    cen["cfgs"] = sorted({tuple(g) for c in codes for g in c["cfgs"]})
    return cen


def encode(px, distance=1.0, lossless=False, strategy_mode=0, fixed_strategy=0, seed=1, epf_iters=-1, gaborish=True,
           container=True, adaptive_lf_smoothing=True, lossless_predictor=6, lossless_squeeze=False, num_threads=8, exif=None,
           xmp=None, lossless_tree=0, bits=8, orientation=1, float_samples=0, colour=0, icc=None, cmyk=False, animation_frames=1, custom_quant_tables=False, prefix_codes=False, lz77=False, num_passes=1, custom_orders=False, lf_contexts=False, palette=False, mislabel_afv=False,
           premultiplied_alpha=False, wide_codes=False, side_info=None, tree=None, alpha_tree=None, lf_tree=None, transforms=None, entropy=None,
           varblocks=None, varblock_sequence=None):
    """px: uint8 array (h, w, nch) with nch in 1..4 (Gray, GrayA, RGB, RGBA); with bits > 8 (up to 16) a uint16 array whose
    samples use the low `bits` bits; with float_samples = 16 / 32 a float16 / float32 array (nominal range [0, 1]).  Returns bytes.
    side_info: dict of make_side_info's keyword arguments (lossy frames: varying maps and custom header parameters).
    tree / alpha_tree / lf_tree: an explicit MA tree for a lossless frame / for the alpha channel / for each LF channel of a lossy frame:
    a list of nodes (property or -1, split value, child for property > split value, other child, predictor, offset, multiplier), node 0
    the root, children after their parent (oracle/jxo_codec.h: EncodeParams::tree).
    wide_codes: the frame's plain ANS codes are written with log_alpha 8 and up to 255 clusters (used contexts are not merged while they
    fit); tokens, contexts and quantised data are those of the same call without it.
    transforms: lossless frames only, integer samples: the frame's transform list in place of the writer's own choice (an OracleError
    together with palette or lossless_squeeze).  Applied forward in order, written to the header in that order; [] is no transform.
    Entries: ("rct", begin_c, rct_type); ("palette", begin_c, num_c), channel indices those of the channel list at that point, the meta
    channels of earlier palettes in front; ("squeeze", [(horizontal, in_place, begin_c, num_c), ...]), an empty list being the default
    parameters (written as a count of 0); and, as the last entry only, ("declare", id, fields...): the header fields of transform `id`
    (0: begin_c, rct_type; 1: begin_c, num_c, nb_colors, nb_deltas, predictor; 2: a list of squeeze tuples) written as given, with nothing
    done to the channels and nothing checked (refusal tests).
    entropy: a dict that changes how the frame's top-level codes turn values into symbols and headers (flatten_entropy); tokens' values
    and contexts and all quantised data are those of the same call without it.  entropy_census() then describes what was written.
    varblocks: lossy frames: [(strategy, bx, by[, raw_quant]), ...], each block at that origin cell, aligned to its size or not; every
    cell left over becomes DCT8.  An OracleError when blocks overlap, leave the frame or cross the edge of their 32x32-cell group.
    varblock_sequence: lossy frames of one LF group, refusal tests: [(strategy, raw_quant), ...] written as the strategy and quant rows
    of the block-metadata channel exactly as given, with their number as the count; the rest of the frame is that of the longest prefix
    the placement rule accepts."""
    L = lib()
    if entropy is not None:
        lz77 = lz77 or "lz" in entropy
        flat = np.ascontiguousarray(flatten_entropy(entropy), dtype=np.int32)
        L.jxo_set_next_entropy.argtypes = [C.c_void_p, C.c_size_t]
        if not L.jxo_set_next_entropy(flat.ctypes.data, len(flat)):
            raise OracleError(L.jxo_last_error().decode())
    if float_samples:
        px = np.ascontiguousarray(px, dtype=np.float16 if float_samples == 16 else np.float32)
    else:
        px = np.ascontiguousarray(px, dtype=np.uint8 if bits <= 8 else np.uint16)
    if px.ndim == 2:
        px = px[:, :, None]
    h, w, nch = px.shape
    p = EncodeParams(distance, int(lossless), 7, strategy_mode, fixed_strategy, seed, epf_iters, int(gaborish), int(container),
                     int(adaptive_lf_smoothing), lossless_predictor, int(lossless_squeeze), lossless_tree, num_threads, bits, orientation, float_samples, colour)
    if custom_quant_tables or prefix_codes or lz77 or num_passes > 1 or custom_orders or lf_contexts or palette or mislabel_afv or premultiplied_alpha or wide_codes:
        L.jxo_set_next_flags.argtypes = [C.c_uint32]
        L.jxo_set_next_flags((1 if custom_quant_tables else 0) | (2 if prefix_codes else 0) | (4 if lz77 else 0) | {1: 0, 2: 8, 3: 16}[num_passes] | (32 if custom_orders else 0) | (64 if lf_contexts else 0) | (128 if palette else 0) |
                             (256 if mislabel_afv else 0) | (512 if premultiplied_alpha else 0) | (1024 if wide_codes else 0))
    if side_info:
        L.jxo_set_next_side_info.argtypes = [C.POINTER(SideInfo)]
        L.jxo_side_info_size.restype = C.c_size_t
        assert L.jxo_side_info_size() == C.sizeof(SideInfo), "SideInfo: the ctypes mirror and jxo_codec.h disagree"
        L.jxo_set_next_side_info(C.byref(make_side_info(**side_info)))
    for role, nodes in enumerate((tree, alpha_tree, lf_tree)):
        if nodes is not None:
            flat = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1, 7)
            L.jxo_set_next_tree.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
            L.jxo_set_next_tree(flat.ctypes.data, len(flat), role)
    if transforms is not None:
        flat = np.ascontiguousarray(flatten_transforms(transforms), dtype=np.int32)
        L.jxo_set_next_transforms.argtypes = [C.c_void_p, C.c_size_t]
        L.jxo_set_next_transforms(flat.ctypes.data, len(flat))
    for kind, blocks in enumerate((varblocks, varblock_sequence)):
        if blocks is not None:
            rows = [tuple(b) + (0,) * (4 - len(b)) for b in blocks] if kind == 0 else [tuple(b) for b in blocks]
            flat = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 2 if kind else 4)
            L.jxo_set_next_varblocks.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
            L.jxo_set_next_varblocks(flat.ctypes.data, len(flat), kind)
    if animation_frames > 1:
        L.jxo_set_next_animation.argtypes = [C.c_int]
        L.jxo_set_next_animation(animation_frames)
    if icc or cmyk:
        L.jxo_set_next_icc.argtypes = [C.c_char_p, C.c_size_t, C.c_int]
        L.jxo_set_next_icc(icc, len(icc) if icc else 0, int(cmyk))
    hnd = L.jxo_encode(px.ctypes.data, w, h, nch, C.byref(p), exif, len(exif) if exif else 0, xmp, len(xmp) if xmp else 0)
    if not hnd:
        raise OracleError(L.jxo_last_error().decode())
    try:
        n = L.jxo_bytes_size(hnd)
        return bytes(C.string_at(L.jxo_bytes_data(hnd), n))
    finally:
        L.jxo_bytes_free(hnd)


_PLANE_DTYPES = {"lf_quant": np.int32, "lf": np.float32, "qcoef": np.int32, "xyb_idct": np.float32, "xyb_filtered": np.float32,
                 "strategy": np.uint8, "raw_quant": np.int32, "sharpness": np.uint8, "ytox": np.int8, "ytob": np.int8,
                 "alpha": np.int32}


class Decoded:
    def __init__(self, pixels, w8, h8, planes, exif, xml, epf_iters, icc=b"", cmyk=False):
        self.icc, self.cmyk = icc, cmyk
        self.pixels = pixels
        self.w8, self.h8 = w8, h8
        self.planes = planes
        self.exif, self.xml = exif, xml
        self.epf_iters = epf_iters


def decode(data, num_threads=8, want_dump=False):
    L = lib()
    hnd = L.jxo_decode(data, len(data), num_threads, int(want_dump))
    if not hnd:
        raise OracleError(L.jxo_last_error().decode())
    try:
        w, h, nch, w8, h8 = (C.c_int32() for _ in range(5))
        L.jxo_image_info(hnd, w, h, nch, w8, h8)
        n = w.value * h.value * nch.value
        L.jxo_image_bits_out.restype = C.c_int32
        L.jxo_image_bits_out.argtypes = [C.c_void_p]
        L.jxo_image_out_float.restype = C.c_int32
        L.jxo_image_out_float.argtypes = [C.c_void_p]
        bo, fl = L.jxo_image_bits_out(hnd), L.jxo_image_out_float(hnd)
        dt = {(8, 0): np.uint8, (16, 0): np.uint16, (16, 1): np.float16, (32, 1): np.float32}[(bo, fl)]
        px = np.ctypeslib.as_array(L.jxo_image_pixels(hnd), shape=(n * (bo // 8),)).view(dt).reshape(h.value, w.value, nch.value).copy()
        planes = {}
        if want_dump:
            for name, dt in _PLANE_DTYPES.items():
                chans = 3 if name in ("lf_quant", "lf", "qcoef", "xyb_idct", "xyb_filtered") else 1
                out = []
                for c in range(chans):
                    ptr, es = C.c_void_p(), C.c_int32()
                    cnt = L.jxo_image_plane(hnd, name.encode(), c, C.byref(ptr), C.byref(es))
                    if cnt == 0:
                        out.append(np.zeros(0, dt))
                    else:
                        buf = (C.c_uint8 * (cnt * es.value)).from_address(ptr.value)
                        out.append(np.frombuffer(buf, dtype=dt).copy())
                planes[name] = out if chans == 3 else out[0]
        if want_dump:
            L.jxo_image_mod_coded_count.argtypes = [C.c_void_p]
            L.jxo_image_mod_coded.restype = C.POINTER(C.c_int32)
            L.jxo_image_mod_coded.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
            coded = []
            for i in range(L.jxo_image_mod_coded_count(hnd)):
                cw, ch = C.c_int32(), C.c_int32()
                ptr = L.jxo_image_mod_coded(hnd, i, C.byref(cw), C.byref(ch))
                if cw.value * ch.value:
                    coded.append(np.ctypeslib.as_array(ptr, shape=(ch.value, cw.value)).copy())
                else:
                    coded.append(np.zeros((ch.value, cw.value), np.int32))
            planes["mod_coded"] = coded   # Modular frames: the coded channel list before the inverse transforms, each (h, w)
        p = C.POINTER(C.c_uint8)()
        n = L.jxo_image_exif(hnd, C.byref(p))
        exif = bytes(C.string_at(p, n)) if n else b""
        n = L.jxo_image_xml(hnd, C.byref(p))
        xml = bytes(C.string_at(p, n)) if n else b""
        L.jxo_image_icc.restype = C.c_size_t
        L.jxo_image_icc.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint8))]
        L.jxo_image_cmyk.argtypes = [C.c_void_p]
        n = L.jxo_image_icc(hnd, C.byref(p))
        icc = bytes(C.string_at(p, n)) if n else b""
        return Decoded(px, w8.value, h8.value, planes, exif, xml, L.jxo_image_epf_iters(hnd), icc, bool(L.jxo_image_cmyk(hnd)))
    finally:
        L.jxo_image_free(hnd)
