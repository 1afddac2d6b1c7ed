"""Reduced-size decode on the GPU (decoder option "downscale" = 8, DESIGN.md §2 "Reduced-size decode"): one pixel per 8x8 cell.

Lossy frames against the float64 reference of rule 1 applied to the oracle's LF dump (DESIGN.md §7's standing tolerance, counted as
tests/test_gpu_noise.py counts it) and against the cell means of the oracle's alpha dump; lossless frames against the cell means of
the SOURCE pixels, exactly.  Every decode goes into a full-size, sentinel-filled buffer (downscale_util.decode_reduced_batch)."""
import math

import numpy as np
import pytest

import downscale_util as DU
import layer_util as LU
import noise_util as NU
import patch_util as PU
from gpu_helpers import gpu_decode
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth, synth16

pytestmark = pytest.mark.gpu

MAX_FRAC_DIFF = 0.002


def check_u8(got, ref, what=""):
    d = np.abs(got.astype(int) - ref.astype(int))
    n_off, n = int((d > 0).sum()), d.size
    print("%s: max %d LSB, %d of %d samples differ (%.4f %%)" % (what, d.max(), n_off, n, 100.0 * n_off / n))
    assert d.max() <= 1, (what, int(d.max()))
    allowed = max(1, math.ceil(MAX_FRAC_DIFF * n)) if n < 1000 else MAX_FRAC_DIFF * n
    assert n_off <= allowed, (what, n_off, n)


# ---------------------------------------------------------------- 1. option values
def test_option_values(oracle, gpu_decoder):
    dec = gpu_decoder
    data = oracle.encode(synth(23, 9, 1)[..., :3], distance=1.0)
    assert dec.set_option("downscale", 8) == 1
    try:
        for bad in (0, 2, 4, 16, -8):
            assert dec.set_option("downscale", bad) == 0
            # the previous value (8) is kept: the next decode is a reduced one
            import torch
            out = torch.full((23 * 9 * 3,), DU.SENTINEL, dtype=torch.uint8, device="cuda")
            assert dec.decode_batch([data], [out.data_ptr()]) == [0]
            assert (out.cpu().numpy()[3 * 2 * 3:] == DU.SENTINEL).all(), bad
        assert dec.set_option("downscale", 1) == 1
        assert dec.set_option("downscale", 2) == 0
        assert gpu_decode(dec, [data])[0].shape == (9, 23, 3)   # ... and the previous value (1) is kept
    finally:
        dec.set_option("downscale", 1)


# ---------------------------------------------------------------- 2. opaque lossy frames
SHAPES = [(5, 3), (8, 8), (9, 9), (23, 9), (257, 300), (600, 400), (2056, 24)]
VARIANTS = {"gab0-epf0": ((300, 280), dict(gaborish=False, epf_iters=0)), "epf3-d4": ((300, 280), dict(distance=4.0, epf_iters=3)),
            "three-passes": ((300, 280), dict(num_passes=3)), "large-varblocks": ((600, 400), dict(strategy_mode=0))}


def _lossy_case(oracle, dec, img, what, **kw):
    data = oracle.encode(img, **dict(dict(distance=1.0), **kw))
    od = oracle.decode(data, want_dump=True)
    got = DU.decode_reduced(dec, data)
    h, w = img.shape[:2]
    assert got.shape == ((h + 7) // 8, (w + 7) // 8, img.shape[2]) and got.dtype == np.uint8
    check_u8(got[..., :3], DU.reference_colour(od), what)
    return od, got


@pytest.mark.parametrize("smoothing", [True, False], ids=["smooth", "no-smooth"])
@pytest.mark.parametrize("w,h", SHAPES)
def test_opaque_lossy(oracle, gpu_decoder, w, h, smoothing):
    _lossy_case(oracle, gpu_decoder, synth(w, h, 3)[..., :3], "%dx%d smoothing=%s" % (w, h, smoothing), adaptive_lf_smoothing=smoothing)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_opaque_lossy_variants(oracle, gpu_decoder, variant):
    (w, h), kw = VARIANTS[variant]
    img = synth(w, h, 5)[..., :3]
    if variant == "large-varblocks":
        # smooth content: the oracle's default strategy mode then places 32x32 and 64x64 varblocks (checked below)
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([xx * 255 // w, yy * 255 // h, (xx + yy) * 255 // (w + h)], axis=2).astype(np.uint8)
    od, _ = _lossy_case(oracle, gpu_decoder, img, variant, **kw)
    if variant == "large-varblocks":
        first = od.planes["strategy"][(od.planes["strategy"] & 0x80) != 0] & 0x7F
        assert (first == 5).any() and (first == 18).any(), sorted(set(first.tolist()))   # DCT32X32 and DCT64X64 (strategy ids)


# ---------------------------------------------------------------- 3. RGBA lossy frames
@pytest.mark.parametrize("w,h", [(9, 9), (200, 150), (257, 300), (600, 400)])
def test_rgba_lossy(oracle, gpu_decoder, w, h):
    img = synth(w, h, 7)
    od, got = _lossy_case(oracle, gpu_decoder, img, "rgba %dx%d" % (w, h))
    alpha = od.planes["alpha"].reshape(h, w)
    assert (alpha == img[..., 3]).all()
    assert np.array_equal(got[..., 3], DU.box_mean_int(alpha.astype(np.uint8)))


def test_rgba_lossy_premultiplied(oracle, gpu_decoder):
    """Associated alpha: the colour of the LF image as coded, divided by max(reduced alpha, 2^-26) on the encoded samples.  alpha >=
    128 / 255 here, so the division at most doubles the conversion's error: the standing tolerance of one step becomes two, and
    the share beyond ONE step stays within 0.2 %."""
    w, h = 257, 300
    img = synth(w, h, 8)
    img[..., 3] = 128 + img[..., 3] // 2
    pm = img.copy()
    pm[..., :3] = np.round(img[..., :3].astype(np.float64) * (img[..., 3:4] / 255.0)).astype(np.uint8)
    data = oracle.encode(pm, distance=1.0, premultiplied_alpha=True)
    od = oracle.decode(data, want_dump=True)
    got = DU.decode_reduced(gpu_decoder, data)
    a = DU.box_mean_int(od.planes["alpha"].reshape(h, w).astype(np.uint8))
    assert np.array_equal(got[..., 3], a)
    lf = np.stack([np.asarray(od.planes["lf"][c], np.float64).reshape(od.h8, od.w8) for c in range(3)])
    ref = NU.to_samples(NU.xyb_to_srgb(lf) / np.maximum(a[..., None] / 255.0, 2.0 ** -26), np.uint8)
    d = np.abs(got[..., :3].astype(int) - ref.astype(int))
    print("premultiplied: max %d LSB, share > 1: %.5f, share > 0: %.5f" % (d.max(), (d > 1).mean(), (d > 0).mean()))
    assert d.max() <= 2 and (d > 1).mean() <= MAX_FRAC_DIFF


# ---------------------------------------------------------------- 4. stages
PIXEL_STAGES = ("reconstruct", "reconstruct_generic", "noise", "filters+output")


def test_stages_that_do_not_run_leave_no_entry(oracle, gpu_decoder):
    img = synth(300, 280, 9)
    DU.decode_reduced(gpu_decoder, oracle.encode(img[..., :3], distance=1.0))
    st = gpu_decoder.stage_times()
    print(st)
    assert "lf_ans" in st and "lf_output" in st
    assert not any(k in st for k in ("hf_decode",) + PIXEL_STAGES), st
    DU.decode_reduced(gpu_decoder, oracle.encode(img, distance=1.0))
    st = gpu_decoder.stage_times()
    print(st)
    assert "hf_decode" in st and "alpha_ans" in st and "lf_output" in st
    assert not any(k in st for k in PIXEL_STAGES), st


# ---------------------------------------------------------------- 5. deeper outputs
@pytest.mark.parametrize("kind", ["u16", "f16", "f32"])
def test_deeper_outputs(oracle, gpu_decoder, kind):
    """The tolerances tests/test_gpu_formats.py holds each type to against the oracle, here against rule 1 in float64.  Alpha is coded
    losslessly: integers exact; floats an f32 sum of at most 64 samples and one division (+ the rounding to binary16)."""
    w, h = 257, 300
    if kind == "u16":
        px, kw, dt = synth16(w, h, 5), dict(bits=16), np.uint16
    else:
        px = synth(w, h, 5).astype(np.float32) / 255
        px, kw, dt = (px, dict(float_samples=32), np.float32) if kind == "f32" else (px.astype(np.float16), dict(float_samples=16), np.float16)
    data = oracle.encode(px, distance=1.0, **kw)
    od = oracle.decode(data, want_dump=True)
    got = DU.decode_reduced(gpu_decoder, data)
    assert got.dtype == dt and got.shape == (38, 33, 4)
    ref = DU.reference_colour(od, dt)
    if kind == "u16":
        d = np.abs(got[..., :3].astype(np.int32) - ref.astype(np.int32))
        print("u16: max %d, share > 8: %.5f" % (d.max(), (d > 8).mean()))
        assert d.max() <= 48 and (d > 8).mean() < 0.002
        assert np.array_equal(got[..., 3], DU.box_mean_int(px[..., 3]))
    else:
        d = np.abs(got[..., :3].astype(np.float32) - ref.astype(np.float32))
        print("%s: max %.3g" % (kind, d.max()))
        assert d.max() < (1e-3 if kind == "f32" else 2e-3)
        mean = DU.box_mean_float(px[..., 3])
        top = float(np.abs(px[..., 3].astype(np.float64)).max())
        bound = 64 * 2.0 ** -24 * top + (2.0 ** -11 * top if kind == "f16" else 0.0)
        assert np.abs(got[..., 3].astype(np.float64) - mean).max() <= bound


# ---------------------------------------------------------------- 6. orientations
_ORIENT = {1: lambda a: a, 2: lambda a: a[:, ::-1], 3: lambda a: a[::-1, ::-1], 4: lambda a: a[::-1], 5: lambda a: a.transpose(1, 0, 2),
           6: lambda a: np.rot90(a, -1), 7: lambda a: a[::-1, ::-1].transpose(1, 0, 2), 8: lambda a: np.rot90(a, 1)}


@pytest.fixture(scope="module")
def upright_23x9(oracle, gpu_decoder):
    img = synth(23, 9, 11)
    return img, DU.decode_reduced(gpu_decoder, oracle.encode(img, distance=1.0)), DU.decode_reduced(gpu_decoder, oracle.encode(img, lossless=True))


@pytest.mark.parametrize("orientation", range(1, 9))
def test_orientations(oracle, gpu_decoder, upright_23x9, orientation):
    img, lossy1, lossless1 = upright_23x9
    got = DU.decode_reduced(gpu_decoder, oracle.encode(img, distance=1.0, orientation=orientation))
    assert np.array_equal(got, _ORIENT[orientation](lossy1))
    got = DU.decode_reduced(gpu_decoder, oracle.encode(img, lossless=True, orientation=orientation))
    assert np.array_equal(got, _ORIENT[orientation](lossless1))
    assert np.array_equal(lossless1, DU.box_mean_int(img))


# ---------------------------------------------------------------- 7. lossless files
def _kind(img, kind):
    return np.ascontiguousarray({"rgb": img[..., :3], "rgba": img, "gray": img[..., 1:2], "graya": img[..., [1, 3]]}[kind])


@pytest.mark.parametrize("w,h", [(9, 9), (257, 300)])
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("kind", ["rgb", "rgba", "gray", "graya"])
def test_lossless_kinds(oracle, gpu_decoder, kind, bits, w, h):
    src = _kind(synth(w, h, 21) if bits == 8 else synth16(w, h, 21), kind)
    got = DU.decode_reduced(gpu_decoder, oracle.encode(src, lossless=True, bits=bits, lossless_tree=1, lossless_predictor=5))
    assert got.dtype == src.dtype and np.array_equal(got, DU.box_mean_int(src))


@pytest.mark.parametrize("w,h", [(9, 9), (257, 300)])
@pytest.mark.parametrize("alpha", [False, True])
def test_lossless_cmyk(oracle, gpu_decoder, alpha, w, h):
    import icc_util
    rng = np.random.default_rng(56)
    base = synth(w, h, 56)
    k = rng.integers(0, 256, (h, w, 1), dtype=np.uint8)
    stored = np.ascontiguousarray(np.concatenate([base[..., :3], k] + ([base[..., 3:4]] if alpha else []), axis=2))
    want = stored.copy()
    want[..., :4] = 255 - want[..., :4]   # the host's ink convention: the mean is taken on the samples the host receives
    got = DU.decode_reduced(gpu_decoder, oracle.encode(stored, lossless=True, icc=icc_util.cmyk_profile(), cmyk=True))
    assert np.array_equal(got, DU.box_mean_int(want))


@pytest.mark.parametrize("variant", ["squeeze", "palette", "weighted"])
def test_lossless_variants(oracle, gpu_decoder, variant):
    w, h = 257, 300
    if variant == "palette":
        rng = np.random.default_rng(3)
        cols = rng.integers(0, 256, (17, 4), dtype=np.uint8)
        yy, xx = np.mgrid[0:h, 0:w]
        src = np.ascontiguousarray(cols[(xx // 7 + yy // 5 + (xx * yy) // 977) % 17])
        data = oracle.encode(src, lossless=True, palette=True)
    else:
        src = synth(w, h, 37)
        data = oracle.encode(src, lossless=True, lossless_squeeze=True) if variant == "squeeze" else oracle.encode(src, lossless=True, lossless_predictor=6)
    assert np.array_equal(DU.decode_reduced(gpu_decoder, data), DU.box_mean_int(src))


def test_lossless_f32(oracle, gpu_decoder):
    """Non-negative float samples: |got - float64 mean| <= 64 * 2^-24 * max |sample of the cell| (63 roundings of the running sum, one
    of the division)."""
    w, h = 257, 300
    src = (synth(w, h, 33)[..., :3].astype(np.float32) / 255.0).astype(np.float32)
    src[10:40, 10:60] *= 1e-3
    got = DU.decode_reduced(gpu_decoder, oracle.encode(src, lossless=True, float_samples=32, lossless_predictor=5, lossless_tree=1))
    assert got.dtype == np.float32
    top = np.zeros((38 * 8, 33 * 8, 3))
    top[:h, :w] = np.abs(src)
    top = top.reshape(38, 8, 33, 8, 3).max(axis=(1, 3))
    err = np.abs(got.astype(np.float64) - DU.box_mean_float(src))
    print("f32: max error / bound = %.3g" % (err / np.maximum(64 * 2.0 ** -24 * top, 1e-300)).max())
    assert (err <= 64 * 2.0 ** -24 * top).all()


# ---------------------------------------------------------------- 8. batches
def _layered(oracle):
    rng = np.random.default_rng(13)
    kw = dict(lossless=True, container=False)
    px = lambda w, h: rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    return LU.layered(oracle.encode(np.zeros((40, 60, 4), np.uint8), **kw),
                      [LU.Layer(oracle.encode(px(60, 40), **kw), crop=False), LU.Layer(oracle.encode(px(20, 20), **kw), x0=5, y0=5)])


def test_batch_of_different_kinds(oracle, gpu_decoder):
    files = [oracle.encode(synth(257, 300, 41)[..., :3], distance=1.0), oracle.encode(synth(200, 150, 42), distance=2.0),
             oracle.encode(synth(9, 9, 43), lossless=True), oracle.encode(synth16(70, 50, 44)[..., 1:2], lossless=True, bits=16),
             oracle.encode(synth(23, 9, 45), distance=1.0, orientation=6)]
    st, together = DU.decode_reduced_batch(gpu_decoder, files)
    assert st == [0] * 5
    for f, t in zip(files, together):
        alone = DU.decode_reduced(gpu_decoder, f)
        assert alone.dtype == t.dtype and np.array_equal(alone, t)


def test_batch_of_more_frames_than_a_pixel_chunk(oracle, gpu_decoder):
    assert gpu_decoder.set_option("query_pixel_chunk", 0) < 33
    kinds = [oracle.encode(synth(40, 24, 51), distance=1.0), oracle.encode(synth(17, 33, 52)[..., :3], distance=1.0), oracle.encode(synth(24, 16, 53), lossless=True)]
    alone = [DU.decode_reduced(gpu_decoder, f) for f in kinds]
    st, got = DU.decode_reduced_batch(gpu_decoder, [kinds[i % 3] for i in range(33)])
    assert st == [0] * 33
    for i, g in enumerate(got):
        assert np.array_equal(g, alone[i % 3]), i


def test_layered_file_in_a_batch_fails_alone(oracle, gpu_decoder):
    files = [oracle.encode(synth(40, 24, 61), distance=1.0), _layered(oracle), oracle.encode(synth(24, 16, 62), lossless=True)]
    st, got = DU.decode_reduced_batch(gpu_decoder, files)
    assert st[0] == 0 and st[2] == 0 and st[1] != 0, st
    assert "downscale 8: layered images are not supported" in gpu_decoder.last_error, gpu_decoder.last_error
    assert np.array_equal(got[0], DU.decode_reduced(gpu_decoder, files[0])) and np.array_equal(got[2], DU.decode_reduced(gpu_decoder, files[2]))


# ---------------------------------------------------------------- 9. back to full size
def test_back_to_full_size(oracle, gpu_decoder):
    files = [oracle.encode(synth(257, 300, 71), distance=1.0), oracle.encode(synth(23, 9, 72)[..., :3], distance=1.0),
             oracle.encode(synth(600, 400, 73), lossless=True)]
    fresh = api.Decoder(0)
    try:
        never = gpu_decode(fresh, files)
    finally:
        fresh.close()
    assert gpu_decoder.set_option("downscale", 1) == 1
    for a, b in zip(gpu_decode(gpu_decoder, files), never):
        assert np.array_equal(a, b)
    DU.decode_reduced_batch(gpu_decoder, files)   # 8, then back to 1
    for a, b in zip(gpu_decode(gpu_decoder, files), never):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- 10. refusals and noise
def _refused(dec, data, needle):
    st, got = DU.decode_reduced_batch(dec, [data])
    assert st[0] != 0 and got[0] is None
    assert needle in dec.last_error, dec.last_error


def test_layered_file_is_refused(oracle, gpu_decoder):
    _refused(gpu_decoder, _layered(oracle), "downscale 8: layered images are not supported")
    assert gpu_decode(gpu_decoder, [_layered(oracle)])[0].shape == (40, 60, 4)   # and still decodes at full size


def test_file_with_patches_is_refused(oracle, gpu_decoder):
    kw = dict(lossless=True, container=False)
    rng = np.random.default_rng(5)
    atlas = rng.integers(0, 128, (11, 20, 3), dtype=np.uint8)
    coded = rng.integers(0, 128, (40, 60, 3), dtype=np.uint8)
    refs = [PU.Ref(0, 1, 1, 7, 9, [PU.Place(5, 5, [(PU.REPLACE, 0, False)]), PU.Place(30, 20, [(PU.REPLACE, 0, False)])])]
    f = LU.layered(oracle.encode(np.zeros_like(coded), **kw),
                   [LU.Layer(oracle.encode(atlas, **kw), frame_type=2, save_before_ct=True), LU.Layer(PU.patched(oracle.encode(coded, **kw), refs, 0), crop=False, flags=2)])
    _refused(gpu_decoder, f, "downscale 8: images with patches are not supported")
    assert api.load_image(f).pixels.shape == (40, 60, 3)


def test_band_decode_is_refused(oracle, gpu_decoder):
    data = oracle.encode(synth(300, 280, 81), distance=1.0)
    gpu_decoder.set_option("band_first_row", 0)
    assert gpu_decoder.set_option("band_rows", 1) == 1
    try:
        _refused(gpu_decoder, data, "downscale 8: band decode is not supported")
    finally:
        gpu_decoder.set_option("band_rows", 0)


def test_noise_frame_equals_the_plain_stream(oracle, gpu_decoder):
    cs = oracle.encode(synth(300, 280, 11), container=False)
    plain = DU.decode_reduced(gpu_decoder, cs)
    assert np.array_equal(DU.decode_reduced(gpu_decoder, NU.noisy(cs, list(range(0, 512, 64)))), plain)
