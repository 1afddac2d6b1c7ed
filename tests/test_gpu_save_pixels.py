"""GPU tests of jxlhip_save_pixels (include/jxlfiletypeio.h, Part 3): 8-bit input against SaveImage byte for byte, lossless integers
against ground truth, lossy deep streams against the CPU oracle's decoder and its encoder on the same samples, every named colour
encoding, strided input, progress and cancellation.

The decoders hand out integer samples of 9..15 bits scaled to 16 bits (round(v * 65535 / (2^bits - 1)), test_gpu_formats.py); the
scaling is one to one, so "equal to the source" is checked after scaling back."""
import numpy as np
import pytest

from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth
from save_pixels_util import (GRAY_PROFILES, ORACLE_COLOUR, bgra_view, channels, float_image, nominal, psnr_nominal, u16_image)

pytestmark = pytest.mark.gpu


def unscale(px16, bits):
    """16-bit output samples of a `bits`-bit stream -> the coded integers."""
    if bits == 16:
        return px16
    return np.round(px16.astype(np.float64) * ((1 << bits) - 1) / 65535.0).astype(np.uint16)


# ---------------------------------------------------------------- 1. the bytes of SaveImage
def _soft(w, h, seed, nch):
    return channels(synth(w, h, seed), nch)


@pytest.mark.parametrize("size", [(40, 30), (300, 280)], ids=["40x30", "300x280"])
@pytest.mark.parametrize("nch", [4, 3, 1], ids=["rgba", "rgb", "gray"])
@pytest.mark.parametrize("lossless,effort", [(False, 3), (False, 7), (False, 8), (True, 7), (True, 9)],
                         ids=["lossy3", "lossy7", "lossy8", "lossless7", "lossless9"])
def test_eight_bit_input_writes_the_bytes_of_save_image(size, nch, lossless, effort):
    w, h = size
    px = _soft(w, h, 3, nch)
    ours = api.save_pixels(px, distance=1.0, effort=effort, lossless=lossless)
    info = api.last_save_lossless_info()
    theirs = api.save_image(bgra_view(px), distance=1.0, effort=effort, lossless=lossless)
    assert ours == theirs
    assert info == api.last_save_lossless_info()   # the searched tiers ran for both (or for neither)


# ---------------------------------------------------------------- 2. lossless integers
@pytest.mark.parametrize("size", [(1, 1), (7, 9), (257, 3), (300, 270), (2056, 24)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("bits", [10, 12, 16])
@pytest.mark.parametrize("nch", [1, 2, 3, 4])
def test_lossless_integers_are_exact(oracle, nch, bits, size):
    w, h = size
    px = u16_image(w, h, 7, bits, nch)
    data = api.save_pixels(px, lossless=True, bits=bits)
    assert api.last_save_lossless_info()["tier"] == 0
    od = oracle.decode(data).pixels
    assert od.dtype == np.uint16 and np.array_equal(unscale(od, bits), px)
    got = api.load_image(data)
    assert got.channel_representation == 1 and got.has_transparency == (nch in (2, 4)) and got.format == ("Gray" if nch < 3 else "Rgb")
    assert np.array_equal(unscale(got.pixels, bits), px)
    if bits == 16:
        assert np.array_equal(od, px) and np.array_equal(got.pixels, px)


def test_lossless_16_bit_noise_fills_the_worst_case_section(oracle):
    """257 x 257 RGBA16 uniform noise, 0 and 65535 present: the full group's section is the largest the lossless path can write."""
    rng = np.random.default_rng(5)
    px = rng.integers(0, 65536, (257, 257, 4), dtype=np.uint16)
    px[0, 0] = 0
    px[0, 1] = 65535
    px[1, 0] = [0, 65535, 0, 65535]
    px[1, 1] = [65535, 0, 65535, 0]
    data = api.save_pixels(px, lossless=True)
    assert len(data) > 257 * 257 * 8 * 0.95          # noise does not compress
    assert np.array_equal(oracle.decode(data).pixels, px)
    assert np.array_equal(api.load_image(data).pixels, px)


def test_lossless_deep_input_gets_the_fixed_stream_at_every_effort():
    px = u16_image(300, 270, 9, 16, 4)
    a = api.save_pixels(px, lossless=True, effort=7)
    assert api.last_save_lossless_info()["tier"] == 0
    b = api.save_pixels(px, lossless=True, effort=9)
    assert api.last_save_lossless_info()["tier"] == 0
    assert a == b


# ---------------------------------------------------------------- 3. lossy deep streams
EFFORTS = [(3, 1), (5, 4), (7, 0)]   # effort -> the oracle encoder's strategy_mode with the same transform set (test_gpu_encode.py)

DEEP_INPUTS = {
    "u12-rgba": ("u16", 12, 4, 1.0), "u12-rgb": ("u16", 12, 3, 1.0), "u16-rgba": ("u16", 16, 4, 1.0), "u16-rgb": ("u16", 16, 3, 1.0),
    "f16-rgba": ("f16", 0, 4, 1.0), "f16-rgb": ("f16", 0, 3, 1.0), "f32-rgba": ("f32", 0, 4, 1.0), "f32-rgb": ("f32", 0, 3, 1.0),
    "f32-rgba-above-1": ("f32", 0, 4, 1.6),
}


def _deep_input(name, w, h, seed):
    kind, bits, nch, gain = DEEP_INPUTS[name]
    if kind == "u16":
        return u16_image(w, h, seed, bits, nch), dict(bits=bits), dict(bits=bits)
    dt = np.float16 if kind == "f16" else np.float32
    return float_image(w, h, seed, dt, nch, gain), dict(), dict(float_samples=16 if kind == "f16" else 32)


@pytest.mark.parametrize("effort,mode", EFFORTS, ids=["fast", "squares", "default"])
@pytest.mark.parametrize("size,seed", [((300, 280), 3), ((520, 400), 4)], ids=["300x280", "520x400"])
@pytest.mark.parametrize("name", list(DEEP_INPUTS))
def test_lossy_deep_streams_are_sound(oracle, name, size, seed, effort, mode):
    w, h = size
    px, ours_kw, oracle_kw = _deep_input(name, w, h, seed)
    kind, bits, nch, gain = DEEP_INPUTS[name]
    if gain > 1:
        assert px[..., :3].max() > 1.2
    data = api.save_pixels(px, distance=1.0, effort=effort, **ours_kw)
    od = oracle.decode(data).pixels
    assert od.shape == px.shape and od.dtype == px.dtype
    src = nominal(px, bits or None)
    if nch == 4:   # alpha is exact: integers by value, floats by bit pattern
        if kind == "u16":
            assert np.array_equal(unscale(od[..., 3], bits), px[..., 3])
        else:
            raw = np.uint16 if kind == "f16" else np.uint32
            assert np.array_equal(od[..., 3].view(raw), px[..., 3].view(raw))
    ours = psnr_nominal(nominal(od)[..., :3], src[..., :3])
    ref = oracle.decode(oracle.encode(px, distance=1.0, strategy_mode=mode, **oracle_kw)).pixels
    theirs = psnr_nominal(nominal(ref)[..., :3], src[..., :3])
    print("%s %dx%d effort %d: PSNR %.2f dB, oracle encoder %.2f dB" % (name, w, h, effort, ours, theirs))
    assert ours > theirs - 0.5, (ours, theirs)
    # the product's decoder on the product's file against the oracle's decode: the bounds of test_gpu_formats.py for the type
    got = api.load_image(data)
    assert got.pixels.shape == od.shape and got.pixels.dtype == od.dtype
    assert got.channel_representation == {"u16": 1, "f16": 2, "f32": 3}[kind]
    if kind == "u16":
        d = np.abs(got.pixels.astype(np.int32) - od.astype(np.int32))
        print("max |product - oracle| = %d steps" % d[..., :3].max())
        assert d[..., :3].max() <= 48
        if nch == 4:
            assert d[..., 3].max() == 0
    else:
        d = np.abs(got.pixels[..., :3].astype(np.float32) - od[..., :3].astype(np.float32))
        print("max |product - oracle| = %.3g" % d.max())
        assert d.max() < (1e-3 if kind == "f32" else 2e-3)


# ---------------------------------------------------------------- 4. quantised data against the oracle's encoder
@pytest.mark.parametrize("name", ["u16-rgba", "f32-rgba"])
def test_quantised_data_of_deep_input_matches_the_oracle_encoder(oracle, name):
    """The comparison and the thresholds of test_gpu_encode.py: test_quantised_data_matches_the_oracle_encoder, for a 16-bit and a
    binary32 input at effort 7 (the oracle's strategy_mode 0)."""
    px, ours_kw, oracle_kw = _deep_input(name, 512, 384, 7)
    a = oracle.decode(api.save_pixels(px, distance=1.0, effort=7, **ours_kw), want_dump=True)
    b = oracle.decode(oracle.encode(px, distance=1.0, strategy_mode=0, **oracle_kw), want_dump=True)
    sa, sb = a.planes["strategy"], b.planes["strategy"]
    same = sa == sb
    print("strategy agreement %.5f" % same.mean())
    assert same.mean() > 0.995
    kinds = set(np.unique(sa[sa >= 0x80] & 0x7F).tolist())
    assert len(kinds & {6, 7, 10, 11}) >= 3 and len(kinds & {18, 19, 20}) >= 1 and kinds <= {0, 4, 5, 6, 7, 10, 11, 18, 19, 20}, kinds
    rq = (a.planes["raw_quant"] != b.planes["raw_quant"]) | ~same
    print("raw quant disagreement %.5f" % rq.mean())
    assert rq.mean() < 0.01
    for c in range(3):
        d = np.abs(a.planes["lf_quant"][c].astype(int) - b.planes["lf_quant"][c].astype(int))[same]
        print("LF %d: max %d, rate %.5f" % (c, d.max(), (d > 0).mean()))
        assert d.max() <= 1 and (d > 0).mean() < 0.01
    w8 = a.w8
    cells_ok = ~rq.reshape(-1)
    for c in range(3):
        qa = a.planes["qcoef"][c].reshape(a.h8, 8, w8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
        qb = b.planes["qcoef"][c].reshape(b.h8, 8, w8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
        d = np.abs(qa[cells_ok].astype(int) - qb[cells_ok].astype(int))
        print("HF %d: max %d, rate %.5f" % (c, d.max(), (d > 0).mean()))
        assert d.max() <= 1 and (d > 0).mean() < (0.015 if c == 2 else 0.004), (c, d.max(), (d > 0).mean())


# ---------------------------------------------------------------- 5. every colour encoding
def _profile_input(profile, seed):
    nch = {"LinearGray": 1, "GraySrgbTRC": 2}.get(profile, 3)
    return channels(synth(300, 260, seed), nch)


@pytest.mark.parametrize("profile", api.KNOWN_PROFILE)
def test_every_colour_encoding_lossless(oracle, profile):
    px = _profile_input(profile, 40)
    data = api.save_pixels(px, lossless=True, colour=profile)
    got = api.load_image(data)
    assert got.known_profile == profile and np.array_equal(got.pixels, px)
    assert np.array_equal(oracle.decode(data).pixels, px)


def _lf_against_the_oracle_encoder(oracle, data, px, **oracle_kw):
    a = oracle.decode(data, want_dump=True)
    b = oracle.decode(oracle.encode(px, distance=1.0, strategy_mode=0, **oracle_kw), want_dump=True)
    for c in range(3):
        d = np.abs(a.planes["lf_quant"][c].astype(int) - b.planes["lf_quant"][c].astype(int))
        print("LF %d: max %d, rate %.5f" % (c, d.max() if d.size else 0, (d > 0).mean() if d.size else 0))
        assert d.max() <= 1 and (d > 0).mean() <= 0.01


@pytest.mark.parametrize("profile", api.KNOWN_PROFILE)
def test_every_colour_encoding_lossy(oracle, profile):
    px = _profile_input(profile, 41)
    data = api.save_pixels(px, distance=1.0, colour=profile)
    got = api.load_image(data)
    assert got.known_profile == profile and got.pixels.shape == px.shape
    nc = 3 if px.shape[2] >= 3 else 1
    mae = np.abs(got.pixels[..., :nc].astype(np.float64) - px[..., :nc]).mean()
    print("%s: mean |decoded - source| = %.3f of 255" % (profile, mae))
    assert mae < 6.5
    if px.shape[2] == 2:
        assert np.array_equal(got.pixels[..., 1], px[..., 1])
    _lf_against_the_oracle_encoder(oracle, data, px, colour=ORACLE_COLOUR[profile])


def test_pq_16_bit_lossy(oracle):
    px = u16_image(300, 260, 42, 16, 3)
    data = api.save_pixels(px, distance=1.0, colour="Rec2020PQ")
    got = api.load_image(data)
    assert got.known_profile == "Rec2020PQ" and got.pixels.dtype == np.uint16
    mae = np.abs(got.pixels.astype(np.float64) - px).mean() / 257.0
    print("mean |decoded - source| = %.3f of 255" % mae)
    assert mae < 6.5
    _lf_against_the_oracle_encoder(oracle, data, px, colour=ORACLE_COLOUR["Rec2020PQ"], bits=16)


def test_gray_is_what_srgb_and_linear_srgb_mean_with_one_or_two_channels():
    px = _soft(120, 90, 6, 2)
    assert api.load_image(api.save_pixels(px, lossless=True, colour="Srgb")).known_profile == "GraySrgbTRC"
    assert api.load_image(api.save_pixels(px, lossless=True, colour="LinearSrgb")).known_profile == "LinearGray"
    assert api.save_pixels(px, colour="Srgb") == api.save_pixels(px, colour="GraySrgbTRC")


# ---------------------------------------------------------------- 6. strided input
@pytest.mark.parametrize("kind", ["u8", "u16", "f16", "f32"])
def test_strided_input_gives_the_bytes_of_the_contiguous_copy(kind):
    w, h = 150, 70
    if kind == "u8":
        px = _soft(w, h, 8, 3)
    elif kind == "u16":
        px = u16_image(w, h, 8, 16, 3)
    else:
        px = float_image(w, h, 8, np.float16 if kind == "f16" else np.float32, 4)
    wide = np.zeros((h, w + 13, px.shape[2]), px.dtype)
    wide[:, 5:5 + w] = px
    view = wide[:, 5:5 + w]
    assert not view.flags["C_CONTIGUOUS"]
    assert api.save_pixels(view, distance=1.0) == api.save_pixels(np.ascontiguousarray(px), distance=1.0)
    if px.dtype.kind == "u":
        assert api.save_pixels(view, lossless=True) == api.save_pixels(np.ascontiguousarray(px), lossless=True)


# ---------------------------------------------------------------- 7. progress and cancellation
@pytest.mark.parametrize("lossless", [False, True], ids=["lossy", "lossless"])
def test_progress_values_and_cancellation(lossless):
    px = u16_image(300, 300, 13, 16, 4)
    seen = []
    api.save_pixels(px, lossless=lossless, progress=lambda p: seen.append(p) or True)
    assert seen[0] == 0 and seen[-1] == 95 and seen == sorted(seen) and {5, 15, 25, 30, 90} <= set(seen)
    for stop_at in (0, 20, 60):
        with pytest.raises(api.JxlError) as e:
            api.save_pixels(px, lossless=lossless, progress=lambda p: p < stop_at)
        assert e.value.status == "UserCanceled"


def test_metadata_boxes_travel_with_deep_input(oracle):
    px = float_image(200, 120, 11, np.float32, 4)
    exif = b"\0\0\0\0II*\0" + bytes(range(40))
    xmp = b"<x:xmpmeta xmlns:x='adobe:ns:meta/'/>"
    od = oracle.decode(api.save_pixels(px, exif=exif, xmp=xmp))
    assert od.exif == exif and od.xml == xmp and od.pixels.shape == px.shape
