"""Shared by the edge-size tests of the lossy encoder (test_encode_edges_host.py, test_gpu_encode_edges.py): two pictures that are not
flat at any size down to 1 x 2, the case table, the sample types cut from the pictures, the oracle encoder's file and dump of a case
(computed once per process, never changed), the edge band and the plane comparison.

synth() is one colour at every size up to 7 x 7 (and at 9 x 9 for some seeds): a tiny frame built from it exercises the container and
nothing of the transform path.  ramp_tex, and smooth_edge at the small sizes, are ramps that keep rising to the last column and the
last row - a partial cell padded by replication then differs from one padded with zeros, by mirroring or by wrapping - and differ in
how steep and how rough they are."""
import functools
import math

import numpy as np

from cfl_util import maps_of, tiles_that_agree   # noqa: F401 (used by both test files)
from pdn_jpegxl_amd.synth import synth

# (effort of the product, strategy mode of the oracle's encoder with the same transform set): tests/test_gpu_encode.py
EFFORTS = [(3, 1), (5, 4), (7, 0)]
MODE_OF_EFFORT = dict(EFFORTS)

# w x h, and what each is the smallest instance of (DESIGN.md section 7 holds the same table)
SIZES = [
    (1, 1), (1, 2), (2, 1),        # one sample; ReflectIndex at n = 1 and 2; a cell that is all padding but one or two samples
    (1, 9), (9, 1),                # a one-pixel-wide frame of two cells
    (7, 7), (8, 8), (9, 9),        # just under, at and just over one cell
    (17, 3),                       # three cells across, three rows of samples
    (63, 65), (65, 63),            # a 64 x 64 region with a one-pixel partial cell on one side, a second region one pixel deep on the other
    (72, 8), (8, 72),              # a second region that is one whole cell
    (127, 129),                    # 32 x 32 and 64-point candidates that must be rejected at the edge
    (255, 257), (257, 255),        # the group edge; a second group one pixel deep; a partial cell on the other axis
    (264, 8), (8, 264),            # a second group of one cell; a frame of one cell row
    (2049, 9), (9, 2049),          # the LF-group edge at 2048; a second LF group one cell wide with a partial cell
]
# both pictures at every size: smooth_edge is there for the 16-point and larger shapes at the frame's edge (from 127 x 129 up, and
# the 16 x 8 / 8 x 16 blocks of the strips and the one-pixel-wide frames below that)
SMOOTH_SIZES = list(SIZES)
SMOOTH_FROM = (127, 129)           # from here on (both sides at least these) mode 0 must put a large shape at the edge
CASES = [("ramp_tex", w, h) for w, h in SIZES] + [("smooth_edge", w, h) for w, h in SMOOTH_SIZES]

# The cells whose activity lies within a float32 rounding of a strategy threshold in one encoder and not in the other: at most two
# entries, (picture, w, h, effort) -> (cell x, cell y, threshold); every cell outside that cell's 64 x 64 region is still compared.
# DESIGN.md section 7 gives the reasoning of each entry.
TIES = {}

DEEP_SIZES = [(1, 2), (9, 9), (65, 63), (257, 255), (2049, 9)]
# name -> (sample kind, bits, channels, colour of the product, colour= of the oracle's encoder)
DEEP_FORMS = {
    "u10": ("u16", 10, 4, "Srgb", 0), "u16": ("u16", 16, 4, "Srgb", 0), "f16": ("f16", 0, 4, "Srgb", 0), "f32": ("f32", 0, 4, "Srgb", 0),
    "gray": ("u8", 8, 1, "Srgb", 0), "gray-alpha": ("u8", 8, 2, "Srgb", 0), "rgb": ("u8", 8, 3, "Srgb", 0),
    "f32-pq": ("f32", 0, 3, "Rec2020PQ", 4),
}
CFL_SIZES = [(9, 9), (65, 63), (72, 8), (257, 255)]
LOOP_SIZES = [(9, 9), (65, 63), (257, 255)]
FLOAT_GAIN = 1.15   # colour samples of the float pictures: the red ramp (up to 236 of 255) ends above 1.0 near the last column
RAMP_TEX_AMPS = ((90.0, 40.0), (40.0, 80.0), (60.0, 90.0))


def case_id(case):
    return "%s-%dx%d" % case


def _ramps(w, h, amps, length, peaks):
    """Three channels that rise towards the bottom right corner on every row and every column, steepest at the last column and row
    (amps[c][0] / length levels a column there, amps[c][1] / length a row) and levelling off `length` samples and more away from them:
    channel c ends at peaks[c] in the corner."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((h, w, 3), np.float64)
    for c in range(3):
        out[..., c] = peaks[c] - amps[c][0] * (1.0 - np.exp(-(w - 1 - xx) / length)) - amps[c][1] * (1.0 - np.exp(-(h - 1 - yy) / length))
    return out, xx, yy


def _alpha(xx, yy, seed):
    """Varies from sample to sample, never 0 or 255."""
    return 40 + np.mod(xx * 5 + yy * 3 + seed * 7, 180)


@functools.lru_cache(maxsize=None)
def ramp_tex(w, h, seed):
    """RGBA8: a ramp per colour channel (1.3 to 3 levels a sample at the last column and row, each channel slanted its own way) under a
    texture of +-6 levels, so that the edge cells have non-zero HF coefficients."""
    col, xx, yy = _ramps(w, h, RAMP_TEX_AMPS, 30.0, (230.0, 200.0, 170.0))
    rng = np.random.default_rng([seed, w, h])
    col += rng.integers(-6, 7, (h, w, 3))
    if w * h <= 2:   # one or two samples: the texture must not cancel the ramp's step
        col[-1, -1] = col[0, 0] + (9, 6, 12)
    img = np.empty((h, w, 4), np.uint8)
    img[..., :3] = np.clip(np.rint(col), 0, 255)
    img[..., 3] = _alpha(xx, yy, seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def smooth_edge(w, h, seed):
    """RGBA8, smooth enough for the 16-point and larger shapes in the last column and row of cells: from 127 x 129 up, and at
    2049 x 9 and 9 x 2049, synth(), which has them there (test_encode_edges_host.py asserts it); below, where synth() is flat or nearly
    so, gentle ramps (0.3 to 1 level a sample at the last column and row) with a texture of one level on a quarter of the samples."""
    if w >= SMOOTH_FROM[0] and h >= SMOOTH_FROM[1] or max(w, h) > 2048:
        img = synth(w, h, seed).copy()
    else:
        col, xx, yy = _ramps(w, h, ((30.0, 50.0), (50.0, 15.0), (15.0, 30.0)), 50.0, (220.0, 180.0, 140.0))
        rng = np.random.default_rng([seed, w, h, 1])
        col += (rng.integers(0, 4, (h, w, 3)) == 0)
        if w * h == 2:   # two samples: a step that no rounding removes
            col[-1, -1] = col[0, 0] + (9, 6, 12)
        img = np.empty((h, w, 4), np.uint8)
        img[..., :3] = np.clip(np.rint(col), 0, 255)
        img[..., 3] = _alpha(xx, yy, seed + 1)
    img.setflags(write=False)
    return img


_PICTURES = {"ramp_tex": ramp_tex, "smooth_edge": smooth_edge}


SEEDS = {"ramp_tex": 5, "smooth_edge": 3}   # synth(.., 3) has 16-point and larger shapes in the last cell column and row at every large size


def picture(case):
    name, w, h = case
    return _PICTURES[name](w, h, SEEDS[name])


# cells a varblock covers across / down (log2) by strategy code: the shapes the two encoders use (encode_kernels.hip: e_lcx, e_lcy)
_LCX = {0: 0, 4: 1, 5: 2, 6: 0, 7: 1, 10: 1, 11: 2, 18: 3, 19: 2, 20: 3}
_LCY = {0: 0, 4: 1, 5: 2, 6: 1, 7: 0, 10: 2, 11: 1, 18: 3, 19: 3, 20: 2}


def edge_blocks_with_hf(dump, c=1):
    """(varblocks that reach the last cell column, varblocks that reach the last cell row) with a non-zero quantised HF coefficient of
    channel c.  (The dump keeps a varblock's coefficients in its own cells, lowest scan positions in its first cell.)"""
    h8, w8 = dump.h8, dump.w8
    st = dump.planes["strategy"].reshape(h8, w8)
    nz = (by_cell(dump.planes["qcoef"][c], h8, w8) != 0).sum(1).reshape(h8, w8)
    col = row = 0
    for by, bx in zip(*np.nonzero(st >= 0x80)):
        s = int(st[by, bx] & 0x7F)
        cx, cy = 1 << _LCX[s], 1 << _LCY[s]
        if nz[by:by + cy, bx:bx + cx].any():
            col += bx + cx == w8
            row += by + cy == h8
    return int(col), int(row)


def bgra_of(rgba):
    return np.ascontiguousarray(rgba[..., [2, 1, 0, 3]])


def channels(rgba, nch):
    """Gray | Gray,A | R,G,B | R,G,B,A of an RGBA array (gray: the green channel)."""
    if nch == 1:
        return np.ascontiguousarray(rgba[..., 1:2])
    if nch == 2:
        return np.ascontiguousarray(rgba[..., [1, 3]])
    return np.ascontiguousarray(rgba[..., :nch])


@functools.lru_cache(maxsize=None)
def deep_picture(form, w, h):
    """ramp_tex in the sample type of `form`: the same content scaled.  Returns (samples, keyword arguments of api.save_pixels,
    keyword arguments of the oracle's encoder)."""
    kind, bits, nch, colour, ocolour = DEEP_FORMS[form]
    rgba = ramp_tex(w, h, SEEDS["ramp_tex"])
    if kind == "u8":
        px, kw, okw = channels(rgba, nch), {}, {}
    elif kind == "u16":
        px = channels(np.rint(rgba.astype(np.float64) * (((1 << bits) - 1) / 255.0)).astype(np.uint16), nch)
        kw, okw = dict(bits=bits), dict(bits=bits)
    else:
        f = rgba.astype(np.float64) / 255.0
        f[..., :3] *= FLOAT_GAIN if colour == "Srgb" else 1.0   # (PQ samples stay inside the nominal range)
        px = channels(f, nch).astype(np.float16 if kind == "f16" else np.float32)
        kw, okw = {}, dict(float_samples=16 if kind == "f16" else 32)
    if colour != "Srgb":
        kw["colour"] = colour
        okw["colour"] = ocolour
    px.setflags(write=False)
    return px, kw, okw


def nominal(px, bits=None):
    """Samples on the nominal [0, 1] scale as float64 (decoders hand out 9..15-bit samples scaled to 16 bits)."""
    if px.dtype.kind == "u":
        return px.astype(np.float64) / float((1 << (bits or 8 * px.dtype.itemsize)) - 1)
    return px.astype(np.float64)


def colour_of(px):
    return px[..., :px.shape[2] - 1] if px.shape[2] in (2, 4) else px


def band_mask(w, h):
    """The last 8 columns and the last 8 rows (a partial cell lies inside them); the whole frame when it has fewer than 1000 samples."""
    m = np.zeros((h, w), bool)
    if w * h < 1000:
        m[:] = True
    else:
        m[:, max(0, w - 8):] = True
        m[max(0, h - 8):, :] = True
    return m


def band_rms(decoded, source, bits=None):
    """RMS error of the colour channels over the band, in units of 255 (nominal scale x 255)."""
    h, w = source.shape[:2]
    m = band_mask(w, h)
    sbits = bits if source.dtype.kind == "u" else None
    e = (nominal(colour_of(decoded))[m] - nominal(colour_of(source), sbits)[m]) * 255.0
    return float(np.sqrt(np.mean(e ** 2)))


def db_of_rms(rms):
    return 99.0 if rms == 0 else 20.0 * math.log10(255.0 / rms)


@functools.lru_cache(maxsize=None)
def oracle_file(case, mode, fitted=False):
    import oracle_lib
    return oracle_lib.encode(picture(case), distance=1.0, strategy_mode=mode, side_info=dict(cfl="fitted") if fitted else None)


@functools.lru_cache(maxsize=None)
def oracle_dump(case, mode, fitted=False):
    import oracle_lib
    return oracle_lib.decode(oracle_file(case, mode, fitted), want_dump=True)


@functools.lru_cache(maxsize=None)
def oracle_deep_dump(form, w, h, mode):
    import oracle_lib
    px, _, okw = deep_picture(form, w, h)
    return oracle_lib.decode(oracle_lib.encode(px, distance=1.0, strategy_mode=mode, **okw), want_dump=True)


def by_cell(plane, h8, w8):
    """A (h8 * 8, w8 * 8) coefficient plane of the oracle's dump as (cells, 64)."""
    return plane.reshape(h8, 8, w8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)


# test_quantised_data_matches_the_oracle_encoder: the share of values that may differ by the one step the hard rule allows
LIMIT_HF, LIMIT_HF_B, LIMIT_LF, LIMIT_STRATEGY = 0.004, 0.015, 0.01, 0.005


def within(count, share, n):
    """Whether `count` of n compared values may differ by one step: fewer than the share, or at most max(1, ceil(share * n)) values for
    a plane of fewer than 1000 values (the rule of DESIGN.md section 7 for small frames; a share of a handful of values would forbid a
    single rounding tie)."""
    return count <= max(1, math.ceil(share * n)) if n < 1000 else count < share * n


def compare_planes(a, b, effort, what, tie=None):
    """The comparison of test_quantised_data_matches_the_oracle_encoder between two dumps (a: the product's file, b: the oracle
    encoder's).  tie: (cell x, cell y) of a TIES entry - the cells of its 64 x 64 region are left out of every plane.  Prints each
    figure before it asserts; returns the figures."""
    assert (a.h8, a.w8) == (b.h8, b.w8), what
    h8, w8 = a.h8, a.w8
    keep = np.ones((h8, w8), bool)
    if tie is not None:
        rx, ry = tie[0] // 8 * 8, tie[1] // 8 * 8
        keep[ry:ry + 8, rx:rx + 8] = False
    keep = keep.reshape(-1)
    sa, sb = a.planes["strategy"].reshape(-1), b.planes["strategy"].reshape(-1)
    assert sa.size == h8 * w8 and sb.size == sa.size, what
    same = (sa == sb)
    ncell = int(keep.sum())
    fig = {"cells": ncell, "strategy": int((~same & keep).sum())}
    print("%s: %d cells, strategy differs in %d" % (what, ncell, fig["strategy"]))
    if effort == 3:
        assert same.all() and ((sa & 0x7F) == 0).all(), what
    elif h8 * w8 < 1000:
        assert same[keep].all(), (what, fig["strategy"], np.nonzero(~same & keep)[0][:16].tolist())
    else:
        assert within(fig["strategy"], LIMIT_STRATEGY, ncell), (what, fig["strategy"])
    rq = (a.planes["raw_quant"].reshape(-1) != b.planes["raw_quant"].reshape(-1)) | ~same
    fig["raw_quant"] = int((rq & keep).sum())
    print("%s: raw quant or strategy differs in %d cells" % (what, fig["raw_quant"]))
    assert within(fig["raw_quant"], LIMIT_LF, ncell), (what, fig["raw_quant"])
    ok_lf = same & keep
    fig["lf"], fig["hf"] = [], []
    for c in range(3):
        d = np.abs(a.planes["lf_quant"][c].astype(int) - b.planes["lf_quant"][c].astype(int)).reshape(-1)[ok_lf]
        fig["lf"].append((int((d > 0).sum()), d.size))
        print("%s: LF %s max %d, %d of %d differ" % (what, "XYB"[c], d.max() if d.size else 0, (d > 0).sum(), d.size))
        assert d.size and d.max() <= 1 and within(int((d > 0).sum()), LIMIT_LF, d.size), (what, c, int(d.max()), int((d > 0).sum()))
    cells_ok = ~rq & keep
    assert cells_ok.any(), what
    for c in range(3):
        qa = by_cell(a.planes["qcoef"][c], h8, w8)[cells_ok].astype(int)
        qb = by_cell(b.planes["qcoef"][c], h8, w8)[cells_ok].astype(int)
        d = np.abs(qa - qb)
        fig["hf"].append((int((d > 0).sum()), d.size))
        print("%s: HF %s max %d, %d of %d differ (non-zero in the oracle's: %d)" % (what, "XYB"[c], d.max(), (d > 0).sum(), d.size, (qb != 0).sum()))
        assert d.max() <= 1 and within(int((d > 0).sum()), LIMIT_HF_B if c == 2 else LIMIT_HF, d.size), (what, c, int(d.max()), int((d > 0).sum()))
    return fig
