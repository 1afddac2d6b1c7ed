"""Frames smaller than one 8x8 cell, 1 to 3 samples high or wide, and a row or column past the kernels' strip, segment and group
edges: where the loop filters reflect edge rows and columns, the halos wrap and the padding of the last cell is read.  Each set of
parameters is one decode_batch of many frames (the assertion messages name the frame), checked against the CPU oracle.

Bars are those of test_gpu_parity.py (check_report: quantised data and metadata exact, TOL_LF, TOL_XYB; at most MAX_LSB on 8-bit
samples; alpha exact), with one change for small frames: where the parity tests allow a fraction MAX_FRAC_DIFF of the samples to be
off by that one LSB, a frame of fewer than 1000 samples may have max(1, ceil(MAX_FRAC_DIFF * n)) such samples (a fraction of a
handful of samples would forbid a single rounding tie).  Deeper outputs use the bars of test_gpu_formats.py under the same rule.
"""
import math

import numpy as np
import pytest

import layer_util as LU
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth, synth16
from gpu_helpers import compare_stages, gpu_decode
from test_gpu_parity import MAX_FRAC_DIFF, MAX_LSB, check_report

pytestmark = pytest.mark.gpu

LAYOUTS = {"rgba": [0, 1, 2, 3], "rgb": [0, 1, 2], "gray": [1], "graya": [1, 3]}
TINY = [1, 2, 3, 4, 5, 7, 8, 9]


def max_off(n):
    """How many of n samples may differ (by at most the frame's tolerance) from the reference."""
    return max(1, math.ceil(MAX_FRAC_DIFF * n)) if n < 1000 else MAX_FRAC_DIFF * n


def image(w, h, seed, layout="rgba"):
    """synth() with per-pixel noise on the colour channels: the edge rows and columns then differ from their neighbours."""
    img = synth(w, h, seed).astype(np.int32)
    img[..., :3] += np.random.default_rng(seed).integers(-24, 25, (h, w, 3))
    return np.ascontiguousarray(np.clip(img, 0, 255).astype(np.uint8)[..., LAYOUTS[layout]])


def check_px(out, ref, what, tol=MAX_LSB):
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    d = np.abs(out.astype(np.int64) - ref.astype(np.int64))
    assert d.max() <= tol, (what, int(d.max()))
    assert (d > 0).sum() <= max_off(d.size), (what, int((d > 0).sum()), d.size)
    if out.shape[2] in (2, 4):
        assert np.array_equal(out[..., -1], ref[..., -1]), what


def decode_both_forms(dec, files):
    """(default kernels, general streaming kernels only): filter_stream_pairs_kernel takes 8-bit frames of even width >= 8."""
    pairs = gpu_decode(dec, files)
    try:
        assert dec.set_option("no_stream_pairs", 1)
        general = gpu_decode(dec, files)
    finally:
        dec.set_option("no_stream_pairs", 0)
    return pairs, general


def check_forms(pairs, general, layout, what):
    if layout == "rgba":
        assert np.array_equal(pairs, general), what   # both forms convert with v_cvt_pk_u8_f32
    else:
        check_px(pairs, general, what)                # the general form's other layouts round half up


# ---------------------------------------------------------------- a. every size up to 9 x 9, every layout and loop-filter setting
@pytest.mark.parametrize("epf,gab", [(0, True), (1, True), (2, True), (3, True), (1, False)])
@pytest.mark.parametrize("layout", ["rgba", "rgb", "gray", "graya"])
def test_lossy_frames_up_to_nine_pixels(gpu_decoder, oracle, layout, epf, gab):
    sizes = [(w, h) for w in TINY for h in TINY]
    files = [oracle.encode(image(w, h, 7 * w + h, layout), distance=2.0, epf_iters=epf, gaborish=gab) for w, h in sizes]
    refs = [oracle.decode(f, want_dump=True) for f in files]
    assert all(r.epf_iters == epf for r in refs)
    pairs, general = decode_both_forms(gpu_decoder, files)
    staged = gpu_decode(gpu_decoder, files, taps=True)     # the stage kernels (the taps switch the streaming kernels off)
    for i, (w, h) in enumerate(sizes):
        what = (w, h)
        check_report(compare_stages(gpu_decoder, i, refs[i]))
        check_px(pairs[i], refs[i].pixels, what)
        check_px(staged[i], refs[i].pixels, what)
        check_px(pairs[i], staged[i], what)
        check_forms(pairs[i], general[i], layout, what)


# ---------------------------------------------------------------- b. short and wide, narrow and tall
WIDE = [(w, h) for h in (1, 2, 3) for w in (8, 10, 118, 120, 121, 122, 124, 240, 241, 242, 248, 249, 250, 256, 257, 2049)]
TALL = [(w, h) for w in (1, 2, 3, 7, 8, 9) for h in (127, 128, 129, 130, 131, 257, 2049)]


@pytest.mark.parametrize("distance,strategy_mode", [(1.0, 0), (2.5, 0), (1.0, 2)], ids=["d1", "d2.5", "d1-random-varblocks"])
@pytest.mark.parametrize("layout", ["rgba", "gray"])
def test_lossy_strips_one_to_three_pixels_across(gpu_decoder, oracle, layout, distance, strategy_mode):
    """Widths around the 120- and 248-column strips and an LF group at 1 to 3 rows; heights around the 128-row segments, the
    256-row groups and an LF group at 1 to 9 columns.  One and two EPF iterations; random varblocks (up to 64 x 64 where they fit)
    meet the frame edge for the frames at least 16 wide."""
    sizes = [s for s in WIDE + TALL if strategy_mode == 0 or s[0] >= 16]
    files = [oracle.encode(image(w, h, w + 3 * h, layout), distance=distance, strategy_mode=strategy_mode, seed=w + h) for w, h in sizes]
    refs = [oracle.decode(f).pixels for f in files]
    pairs, general = decode_both_forms(gpu_decoder, files)
    for i, s in enumerate(sizes):
        check_px(pairs[i], refs[i], s)
        check_forms(pairs[i], general[i], layout, s)


# ---------------------------------------------------------------- c. deep outputs and orientation at tiny sizes
SMALL = [(1, 5), (5, 1), (2, 3), (3, 2), (1, 1)]
ORIENT = {1: lambda a: a, 2: lambda a: a[:, ::-1], 3: lambda a: a[::-1, ::-1], 4: lambda a: a[::-1], 5: lambda a: a.transpose(1, 0, 2),
          6: lambda a: np.rot90(a, -1), 7: lambda a: a[::-1, ::-1].transpose(1, 0, 2), 8: lambda a: np.rot90(a, 1)}


def test_lossy_16_bit_tiny_frames(oracle):
    for w, h in SMALL:
        px = synth16(w, h, 5 + w * h)
        data = oracle.encode(px, distance=1.0, bits=16)
        got, ref = api.load_image(data), oracle.decode(data)
        assert got.channel_representation == 1 and got.pixels.shape == (h, w, 4), (w, h)
        d = np.abs(got.pixels.astype(np.int32) - ref.pixels.astype(np.int32))[..., :3]
        assert d.max() <= 48 and (d > 8).sum() <= max_off(d.size), (w, h, int(d.max()))
        assert np.array_equal(got.pixels[..., 3], px[..., 3]), (w, h)


@pytest.mark.parametrize("kind", [32, 16])
def test_lossy_float_tiny_frames(oracle, kind):
    rng = np.random.default_rng(kind)
    for w, h in SMALL:
        img = (synth(w, h, 32 + w).astype(np.float32) / 255 + rng.uniform(0, 1e-3, (h, w, 4))).astype(np.float32)
        px = img if kind == 32 else img.astype(np.float16)
        data = oracle.encode(px, distance=1.0, float_samples=kind)
        got, ref = api.load_image(data), oracle.decode(data)
        assert got.pixels.dtype == ref.pixels.dtype == px.dtype and got.pixels.shape == px.shape, (w, h)
        d = np.abs(got.pixels[..., :3].astype(np.float32) - ref.pixels[..., :3].astype(np.float32))
        assert d.max() < (1e-3 if kind == 32 else 2e-3), (w, h, float(d.max()))
        bits = np.uint32 if kind == 32 else np.uint16
        assert np.array_equal(got.pixels[..., 3].view(bits), px[..., 3].view(bits)), (w, h)


@pytest.mark.parametrize("bits", [8, 16])
def test_lossy_premultiplied_tiny_frames(oracle, bits):
    """Per-pixel output path (WritePixelGeneral): un-premultiplied on the way out.  Alpha is kept at a quarter or more, where
    test_premultiplied_alpha_is_undone compares (the division amplifies float differences by 1 / alpha)."""
    maxv = (1 << bits) - 1
    tol = 1 if bits == 8 else 48
    rng = np.random.default_rng(bits)
    for w, h in SMALL:
        img = image(w, h, 12 + w) if bits == 8 else synth16(w, h, 12 + w)
        img[..., 3] = rng.integers(maxv // 4, maxv + 1, (h, w))
        a = img[..., 3:].astype(np.float64) / maxv
        pm = img.copy()
        pm[..., :3] = np.round(img[..., :3].astype(np.float64) * a).astype(img.dtype)
        data = oracle.encode(pm, bits=bits, premultiplied_alpha=True)
        got, ref = api.load_image(data), oracle.decode(data)
        assert got.has_transparency and np.array_equal(got.pixels[..., 3], img[..., 3]), (w, h)
        d = np.abs(got.pixels.astype(np.int64) - ref.pixels.astype(np.int64))[..., :3]
        assert d.max() <= 4 * tol and (d > tol).sum() <= max_off(d.size), (w, h, int(d.max()))


@pytest.mark.parametrize("lossless", [False, True], ids=["lossy", "lossless"])
def test_orientations_of_tiny_frames(gpu_decoder, oracle, lossless):
    """orient_kernel on frames 1 to 5 pixels across, every orientation: against the oracle, and exactly the flip / rotation of the
    decode of the same frame stored upright (lossless: of the source)."""
    kw = dict(lossless=True, lossless_predictor=5, lossless_tree=1) if lossless else dict(distance=1.0)
    cases = [(w, h, o) for w, h in SMALL for o in range(1, 9)]
    srcs = {(w, h): image(w, h, 50 + 2 * w + h) for w, h in SMALL}
    files = [oracle.encode(srcs[w, h], orientation=o, **kw) for w, h, o in cases]
    outs = gpu_decode(gpu_decoder, files)
    upright = {(w, h): outs[i] for i, (w, h, o) in enumerate(cases) if o == 1}
    for i, (w, h, o) in enumerate(cases):
        what = (w, h, o)
        ref = oracle.decode(files[i]).pixels
        if lossless:
            assert np.array_equal(outs[i], ORIENT[o](srcs[w, h])), what
            assert np.array_equal(outs[i], ref), what
        else:
            check_px(outs[i], ref, what)
            assert np.array_equal(outs[i], ORIENT[o](upright[w, h])), what


# ---------------------------------------------------------------- d. lossless at tiny sizes
LOSSLESS_SIZES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (8, 1), (1, 8), (9, 9), (1, 300), (300, 1), (2, 257), (257, 2)]
LOSSLESS_MODES = {"gradient-tree": dict(lossless_tree=1, lossless_predictor=5), "weighted": {}, "squeeze": dict(lossless_squeeze=True),
                  "palette": dict(palette=True)}


@pytest.mark.parametrize("mode", list(LOSSLESS_MODES))
def test_lossless_tiny_frames(gpu_decoder, oracle, mode):
    sizes = LOSSLESS_SIZES
    srcs = [image(w, h, 60 + w + 5 * h) for w, h in sizes]
    if mode == "palette":
        srcs = [np.ascontiguousarray(s // 64 * 64) for s in srcs]   # few colours
    files = [oracle.encode(s, lossless=True, **LOSSLESS_MODES[mode]) for s in srcs]
    outs = gpu_decode(gpu_decoder, files)
    for s, f, o, size in zip(srcs, files, outs, sizes):
        assert np.array_equal(o, s), size
        assert np.array_equal(o, oracle.decode(f).pixels), size


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_lossless_deep_tiny_frames(oracle, kind):
    for w, h in LOSSLESS_SIZES:
        if kind == "u16":
            src = np.ascontiguousarray(synth16(w, h, 70 + w)[..., :3])
            data = oracle.encode(src, lossless=True, bits=16)
        else:
            src = (synth(w, h, 71 + h)[..., :3].astype(np.float32) / 255.0).astype(np.float32)
            data = oracle.encode(src, lossless=True, float_samples=32)
        got = api.load_image(data)
        assert got.pixels.dtype == src.dtype and got.pixels.shape == src.shape, (w, h)
        assert np.array_equal(got.pixels.view(np.uint8), src.view(np.uint8)), (w, h)
        assert np.array_equal(got.pixels.view(np.uint8), oracle.decode(data).pixels.view(np.uint8)), (w, h)


# ---------------------------------------------------------------- e. layered files with thin layers
def test_thin_lossy_replace_layers(oracle):
    """Lossy kReplace layers 1 or 2 rows high or 1 column wide decode through the loop filters at their own size: the file equals
    the standalone decodes placed on the canvas, byte for byte, and each standalone decode matches the oracle."""
    W, H = 61, 37
    parts = [(image(W, H, 81), None), (image(37, 1, 82), (2, 3)), (image(16, 2, 83), (-4, 10)), (image(1, 25, 84), (20, 2)),
             (image(8, 2, 85), (56, 36)), (image(10, 1, 86), (5, 36)), (image(2, 2, 87), (-1, -1)), (image(1, 40, 88), (60, -2))]
    files = [oracle.encode(img, distance=1.0, container=False) for img, _ in parts]
    layers = [LU.Layer(cs, crop=pos is not None, x0=pos[0] if pos else 0, y0=pos[1] if pos else 0) for cs, (_, pos) in zip(files, parts)]
    got = api.load_image(LU.layered(files[0], layers)).pixels
    ref = np.zeros((H, W, 4), np.uint8)
    for cs, (img, pos) in zip(files, parts):
        alone = api.load_image(cs).pixels
        check_px(alone, oracle.decode(cs).pixels, img.shape[:2])
        x0, y0 = pos if pos else (0, 0)
        h, w = alone.shape[:2]
        cx0, cy0, cx1, cy1 = max(0, x0), max(0, y0), min(W, x0 + w), min(H, y0 + h)
        ref[cy0:cy1, cx0:cx1] = alone[cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0]
    assert got.shape == ref.shape and (got == ref).all(), int((got != ref).sum())


def test_lossless_blend_of_one_pixel_layers(oracle):
    """kBlend of 1 x 1 and 1 x N layers (compose_kernel), against the numpy composite of test_gpu_layers."""
    from test_gpu_layers import F, _check, build, composite
    rng = np.random.default_rng(91)
    W, H = 23, 17
    px = lambda w, h: rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    frames = [F(px(W, H), crop=False), F(px(1, 1), x0=4, y0=5, mode=2), F(px(1, 13), x0=22, y0=8, mode=2), F(px(9, 1), x0=-3, y0=0, mode=2),
              F(px(1, 1), x0=0, y0=16, mode=2)]
    got = api.load_image(build(oracle, W, H, frames)).pixels
    _check(got, composite(W, H, frames, 8, True, False), exact=False)


# ---------------------------------------------------------------- f. SaveImage round trips
SAVE_SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (8, 1), (16, 2), (9, 9)]


@pytest.mark.parametrize("distance", [1.0, 2.5])
@pytest.mark.parametrize("effort", [3, 7], ids=["fast", "default"])
def test_save_image_tiny_lossy(oracle, effort, distance):
    for w, h in SAVE_SIZES:
        img = image(w, h, 100 + w + h)
        data = api.save_image(np.ascontiguousarray(img[..., [2, 1, 0, 3]]), distance=distance, effort=effort)
        od = oracle.decode(data)
        assert od.pixels.shape == (h, w, 4) and (od.pixels[..., 3] == img[..., 3]).all(), (w, h)
        check_px(api.load_image(data).pixels, od.pixels, (w, h))


def test_save_image_tiny_lossless(oracle):
    for w, h in SAVE_SIZES:
        img = image(w, h, 110 + w + h)
        data = api.save_image(np.ascontiguousarray(img[..., [2, 1, 0, 3]]), lossless=True)
        assert np.array_equal(oracle.decode(data).pixels, img), (w, h)
        assert np.array_equal(api.load_image(data).pixels, img), (w, h)


# ---------------------------------------------------------------- g. tiny frames beside a large one in one launch
def test_mixed_batch_of_tiny_and_large_frames(gpu_decoder, oracle):
    """About 20 tiny frames and one 600 x 400 frame, interleaved: workgroups past a small image's tasks exit early while the large
    image's run.  Every output is byte-identical to the frame decoded alone."""
    tiny = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 1), (8, 1), (16, 2), (9, 9), (5, 7), (1, 9), (8, 2), (10, 1), (122, 2), (2, 130),
            (3, 3), (7, 1), (1, 3), (4, 4), (248, 1), (257, 2)]
    sizes = tiny[:10] + [(600, 400)] + tiny[10:]
    files = []
    for i, (w, h) in enumerate(sizes):
        img = image(w, h, 120 + i, ["rgba", "rgb", "gray", "graya"][i % 4] if (w, h) != (600, 400) else "rgba")
        files.append(oracle.encode(img, distance=[1.0, 2.5, 4.5][i % 3], epf_iters=3 if i % 3 == 2 else -1))
    batch = gpu_decode(gpu_decoder, files)
    for f, out, s in zip(files, batch, sizes):
        alone = gpu_decode(gpu_decoder, [f])[0]
        assert np.array_equal(out, alone), s
        check_px(out, oracle.decode(f).pixels, s)


# ---------------------------------------------------------------- h. a last band of 1 to 3 rows
@pytest.mark.parametrize("distance", [1.0, 2.5])
def test_bands_ending_in_one_to_three_rows(gpu_decoder, oracle, distance):
    from pdn_jpegxl_amd.distributed import decode_frame_band
    for h in (257, 258, 259):
        data = oracle.encode(image(300, h, 130 + h), distance=distance)
        whole = gpu_decode(gpu_decoder, [data])[0]
        check_px(whole, oracle.decode(data).pixels, h)
        rows = 0
        for rank in range(2):
            band, (y0, y1) = decode_frame_band(gpu_decoder, data, rank, 2)
            assert np.array_equal(band.cpu().numpy().reshape(y1 - y0, 300, 4), whole[y0:y1]), (h, rank, y0, y1)
            rows += y1 - y0
        assert rows == h and y1 - y0 == h - 256, (h, y0, y1)
