"""Synthetic noise on the GPU (frame flag 1): the generator bit for bit and the convolution against the numpy reference of DESIGN.md §2
("Noise: rules restated, not pinned"), the final pixels against that reference applied to the oracle's filtered planes of the plain
stream, and identities that hold whatever the bit-level rules are."""
import math

import numpy as np
import pytest

import layer_util as LU
import noise_util as NU
from gpu_helpers import gpu_decode
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth, synth16

pytestmark = pytest.mark.gpu

FLAT, RAMP, SATURATED = [64] * 8, list(range(0, 512, 64)), [1023] * 8
MAX_FRAC_DIFF = 0.002


def check_u8(got, ref, what=""):
    d = np.abs(got.astype(int) - ref.astype(int))
    n_off, n = int((d > 0).sum()), d.size
    print("%s: max %d LSB, %d of %d samples differ (%.4f %%)" % (what, d.max(), n_off, n, 100.0 * n_off / n))
    assert d.max() <= 1, (what, int(d.max()))
    allowed = max(1, math.ceil(MAX_FRAC_DIFF * n)) if n < 1000 else MAX_FRAC_DIFF * n
    assert n_off <= allowed, (what, n_off, n)


def taps_of(dec, data, index=0):
    """(pixels of every image, R, N) with R / N the (3, h, w) taps of image `index` of the one-file batch."""
    px = gpu_decode(dec, [data], taps=True)
    try:
        R = np.stack([dec.read_plane(index, "noise_rnd", c) for c in range(3)])
        N = np.stack([dec.read_plane(index, "noise", c) for c in range(3)])
    finally:
        dec.set_option("debug_taps", 0)
    return px, R, N


@pytest.mark.parametrize("w,h", [(600, 400), (257, 300), (5, 3)])
def test_random_planes_bit_for_bit_and_convolution(oracle, gpu_decoder, w, h):
    cs = oracle.encode(synth(w, h, 3), container=False)
    _, R, N = taps_of(gpu_decoder, NU.noisy(cs, RAMP))
    want = NU.random_planes(w, h)
    R = R.reshape(3, h, w)
    assert (R.view(np.uint32) == want.view(np.uint32)).all(), int((R.view(np.uint32) != want.view(np.uint32)).sum())
    err = float(np.abs(N.reshape(3, h, w).astype(np.float64) - NU.convolve(want)).max())
    print("%dx%d: max |N - float64 reference| = %.3g" % (w, h, err))
    assert err <= 24 * 2.0 ** -24 * 15.36 * 0.22
    if w > 256:   # no repeated tile
        assert not (R[:, :100, :88] == R[:, :100, 256:344]).all()
        assert np.abs(R[:, :100, :88] - R[:, :100, 256:344]).mean() > 0.2


FILTERS = {"none": dict(gaborish=False, epf_iters=0), "gab": dict(gaborish=True, epf_iters=0), "epf1": dict(epf_iters=1),
           "epf2": dict(epf_iters=2), "epf3": dict(distance=4.0, epf_iters=3)}
CASES = [(f, "ramp", 1, 300, 280) for f in FILTERS] + [("epf1", "flat", 1, 600, 400), ("epf2", "saturated", 1, 300, 280),
                                                         ("epf1", "ramp", 3, 300, 280), ("epf1", "ramp", 1, 257, 300),
                                                         ("none", "flat", 1, 5, 3), ("epf2", "ramp", 1, 23, 9)]


@pytest.mark.parametrize("general", [False, True], ids=["pairs", "no_stream_pairs"])
@pytest.mark.parametrize("filt,lut,passes,w,h", CASES)
def test_pixels_match_the_reference(oracle, gpu_decoder, filt, lut, passes, w, h, general):
    lut10 = {"ramp": RAMP, "flat": FLAT, "saturated": SATURATED}[lut]
    cs = oracle.encode(synth(w, h, 11), container=False, num_passes=passes, **FILTERS[filt])
    od = oracle.decode(cs, want_dump=True)
    ref = NU.reference_pixels(od, w, h, lut10)
    gpu_decoder.set_option("no_stream_pairs", 1 if general else 0)
    try:
        got = gpu_decode(gpu_decoder, [NU.noisy(cs, lut10, passes)])[0]
    finally:
        gpu_decoder.set_option("no_stream_pairs", 0)
    assert (got[..., 3] == od.pixels[..., 3]).all()
    check_u8(got[..., :3], ref, "%s %s passes=%d %dx%d" % (filt, lut, passes, w, h))
    assert (got[..., :3] != od.pixels[..., :3]).mean() > 0.05   # and the noise is there


def test_saturated_noise_on_mid_grey_clips(oracle, gpu_decoder):
    """Every strength 1023 / 1024 on a mid-grey image: a large share of the samples leaves the range, which the output clamps."""
    w, h = 300, 280
    img = np.full((h, w, 4), 127, np.uint8)
    cs = oracle.encode(img, container=False)
    od = oracle.decode(cs, want_dump=True)
    ref = NU.reference_pixels(od, w, h, SATURATED)
    got = gpu_decode(gpu_decoder, [NU.noisy(cs, SATURATED)])[0]
    check_u8(got[..., :3], ref, "mid-grey, saturated")
    clipped = float(((ref == 0) | (ref == 255)).mean())
    print("clipped share %.3f" % clipped)
    assert clipped > 0.2


@pytest.mark.parametrize("kind", ["u16", "f16", "f32"])
def test_deeper_output_types(oracle, kind):
    w, h = 300, 260
    if kind == "u16":
        px, kw, dt = synth16(w, h, 5), dict(bits=16), np.uint16
    else:
        px = synth(w, h, 5).astype(np.float32) / 255
        px, kw, dt = (px, dict(float_samples=32), np.float32) if kind == "f32" else (px.astype(np.float16), dict(float_samples=16), np.float16)
    cs = oracle.encode(px, distance=1.0, container=False, **kw)
    od = oracle.decode(cs, want_dump=True)
    ref = NU.reference_pixels(od, w, h, RAMP, dt)
    got = api.load_image(NU.noisy(cs, RAMP)).pixels
    assert got.dtype == dt
    if kind == "u16":   # the tolerances of tests/test_gpu_formats.py against the oracle for each type
        d = np.abs(got[..., :3].astype(np.int32) - ref.astype(np.int32))
        print("u16: max %d, share > 8: %.5f" % (d.max(), (d > 8).mean()))
        assert d.max() <= 48 and (d > 8).mean() < 0.002
        assert np.array_equal(got[..., 3], px[..., 3])
    else:
        d = np.abs(got[..., :3].astype(np.float32) - ref.astype(np.float32))
        print("%s: max %.3g" % (kind, d.max()))
        assert d.max() < (1e-3 if kind == "f32" else 2e-3)
    assert np.abs(got[..., :3].astype(np.float64) - od.pixels[..., :3].astype(np.float64)).mean() > 0


@pytest.mark.parametrize("general", [False, True], ids=["pairs", "no_stream_pairs"])
@pytest.mark.parametrize("w,nch", [(300, 4), (257, 4), (300, 3), (301, 3), (302, 1)])
def test_zero_strength_is_the_plain_decode(oracle, gpu_decoder, w, nch, general):
    """Every route: the pixel conversion of a noise frame is the one the same frame without noise gets."""
    img = synth(w, 280, 2)
    img = img[..., :3] if nch == 3 else (img[..., 1] if nch == 1 else img)
    gpu_decoder.set_option("no_stream_pairs", 1 if general else 0)
    try:
        # (two iterations without Gaborish: with it, a frame without alpha gets the all-default frame header, which layer_util does
        # not rewrite)
        for kw in (dict(), dict(distance=2.0, epf_iters=2, gaborish=nch == 4), dict(gaborish=False, epf_iters=0), dict(gaborish=True, epf_iters=0),
                   dict(distance=4.0, epf_iters=3)):
            cs = oracle.encode(img, container=False, **kw)
            plain, zero = gpu_decode(gpu_decoder, [cs])[0], gpu_decode(gpu_decoder, [NU.noisy(cs, [0] * 8)])[0]
            assert (plain == zero).all(), (kw, int((plain != zero).sum()))
    finally:
        gpu_decoder.set_option("no_stream_pairs", 0)


def test_repeatable_alone_and_in_a_mixed_batch(oracle, gpu_decoder):
    a = NU.noisy(oracle.encode(synth(600, 400, 1), container=False), RAMP)
    b = NU.noisy(oracle.encode(synth(257, 300, 2), container=False, distance=2.0), FLAT)
    others = [oracle.encode(synth(300, 260, 3), distance=1.0), oracle.encode(synth(200, 150, 4), lossless=True)]
    alone = [gpu_decode(gpu_decoder, [f])[0] for f in (a, b)]
    for stride in (1, 64, 0):
        again = [gpu_decode(gpu_decoder, [f], lane_stride=stride)[0] for f in (a, b)]
        mixed = gpu_decode(gpu_decoder, [others[0], a, others[1], b], lane_stride=stride)
        for k in range(2):
            assert (again[k] == alone[k]).all(), (stride, k)
        assert (mixed[1] == alone[0]).all() and (mixed[3] == alone[1]).all(), stride
        assert (mixed[0] == gpu_decode(gpu_decoder, [others[0]])[0]).all()   # and the plain frame beside them is untouched
    gpu_decoder.set_option("lane_stride", 0)


def test_batch_of_more_frames_than_a_pixel_chunk(oracle, gpu_decoder):
    """Frames share the pixel-stage planes (the noise planes among them) in chunks: a batch of two chunks and a part decodes every
    frame as alone."""
    chunk = gpu_decoder.set_option("query_pixel_chunk", 0)
    assert chunk >= 1
    kinds = [NU.noisy(oracle.encode(synth(90, 70, 1), container=False), RAMP), oracle.encode(synth(80, 60, 2), container=False),
             NU.noisy(oracle.encode(synth(300, 40, 3), container=False, distance=2.0, epf_iters=2), FLAT)]
    alone = [gpu_decode(gpu_decoder, [f])[0] for f in kinds]
    n = 2 * chunk + 5
    got = gpu_decode(gpu_decoder, [kinds[i % 3] for i in range(n)])
    for i in range(n):
        assert (got[i] == alone[i % 3]).all(), i


def test_band_equals_the_rows_of_the_whole_decode(oracle, gpu_decoder):
    import torch
    w, h = 300, 600   # three group rows
    data = NU.noisy(oracle.encode(synth(w, h, 6), container=False), RAMP)
    whole = gpu_decode(gpu_decoder, [data])[0]
    try:
        for first, rows in ((0, 1), (1, 1), (2, 1), (0, 2), (1, 2)):
            y0, y1 = first * 256, min(h, (first + rows) * 256)
            out = torch.zeros((y1 - y0) * w * 4, dtype=torch.uint8, device="cuda")
            assert gpu_decoder.set_option("band_first_row", first) and gpu_decoder.set_option("band_rows", rows)
            st = gpu_decoder.decode_batch([data], [out.data_ptr()])
            assert st[0] == 0
            band = out.cpu().numpy().reshape(y1 - y0, w, 4)
            assert (band == whole[y0:y1]).all(), (first, rows, int((band != whole[y0:y1]).sum()))
    finally:
        gpu_decoder.set_option("band_rows", 0)
        gpu_decoder.set_option("band_first_row", 0)


_ORIENT = {1: lambda a: a, 2: lambda a: a[:, ::-1], 3: lambda a: a[::-1, ::-1], 4: lambda a: a[::-1], 5: lambda a: a.transpose(1, 0, 2),
           6: lambda a: np.rot90(a, -1), 7: lambda a: a[::-1, ::-1].transpose(1, 0, 2), 8: lambda a: np.rot90(a, 1)}


def test_orientations(oracle):
    img = synth(300, 260, 12)
    base = api.load_image(NU.noisy(oracle.encode(img, container=False), RAMP)).pixels
    for o in range(2, 9):
        got = api.load_image(NU.noisy(oracle.encode(img, container=False, orientation=o), RAMP)).pixels
        assert np.array_equal(got, _ORIENT[o](base)), o


@pytest.mark.parametrize("strength,lo,hi", [(64, 4.0, 18.6), (16, 1.0, 4.6)])
def test_flat_grey_gets_zero_mean_noise_of_the_right_size(oracle, strength, lo, hi):
    """Whatever the bit-level rules: the numpy prototype gives a per-channel standard deviation of 9.3 LSB and a mean 0.55 LSB above
    the plain decode for strength 64 (2.3 and 0.5 for 16); a field that is missing, applied twice (twice the deviation: the upper
    bound) or not zero-mean fails this."""
    img = np.full((280, 300, 4), 127, np.uint8)
    cs = oracle.encode(img, container=False)
    plain = api.load_image(cs).pixels.astype(np.float64)
    got = api.load_image(NU.noisy(cs, [strength] * 8)).pixels.astype(np.float64)
    assert (got[..., 3] == plain[..., 3]).all()
    for c in range(3):
        d = got[..., c] - plain[..., c]
        print("strength %d channel %d: std %.2f, mean %.2f" % (strength, c, d.std(), d.mean()))
        assert abs(d.mean()) <= 2.0
        assert lo < d.std() < hi


def _select(W, H, parts):
    ref = np.zeros((H, W, 4), np.uint8)
    for alone, pos in parts:
        x0, y0 = pos if pos else (0, 0)
        h, w = alone.shape[:2]
        cx0, cy0, cx1, cy1 = max(0, x0), max(0, y0), min(W, x0 + w), min(H, y0 + h)
        ref[cy0:cy1, cx0:cx1] = alone[cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0]
    return ref


def test_noise_on_the_first_replace_layer(oracle):
    """A full-canvas lossy layer with noise under a cropped plain one: the numpy selection of the two lone decodes, byte for byte
    (the first frame's indexes are (0, 0), as in its lone file)."""
    W, H = 333, 257
    a, b = oracle.encode(synth(W, H, 21), container=False), oracle.encode(synth(150, 120, 22), container=False)
    data = LU.layered(a, [LU.Layer(NU.with_noise(a, RAMP), crop=False, flags=1), LU.Layer(b, x0=-30, y0=40)])
    got = api.load_image(data).pixels
    ref = _select(W, H, [(api.load_image(NU.noisy(a, RAMP)).pixels, None), (api.load_image(b).pixels, (-30, 40))])
    assert got.shape == ref.shape and (got == ref).all(), int((got != ref).sum())
    assert (got != _select(W, H, [(api.load_image(a).pixels, None), (api.load_image(b).pixels, (-30, 40))])).any()


def test_noise_on_the_second_cropped_layer(oracle, gpu_decoder):
    """The second frame of a layered file follows a frame that is not displayed: seeds (0, 1, x0, y0), groups in its own coordinates."""
    W, H = 333, 257
    w, h = 270, 120   # two groups across
    a, b = oracle.encode(synth(W, H, 21), container=False), oracle.encode(synth(w, h, 22), container=False)
    data = LU.layered(a, [LU.Layer(a, crop=False), LU.Layer(NU.with_noise(b, RAMP), x0=40, y0=100, flags=1)])
    px, R, _ = taps_of(gpu_decoder, data, index=1)
    want = NU.random_planes(w, h, 0, 1)
    assert (R.reshape(3, h, w).view(np.uint32) == want.view(np.uint32)).all()
    assert (want != NU.random_planes(w, h, 0, 0)).any()
    got = api.load_image(data).pixels
    first = api.load_image(a).pixels
    outside = np.ones((H, W), bool)
    outside[100:100 + h, 40:40 + w] = False
    assert (got[outside] == first[outside]).all()
    inside = got[100:100 + h, 40:40 + w][:H - 100, :W - 40]
    plain_b = api.load_image(b).pixels[:H - 100, :W - 40]
    assert (inside[..., :3] != plain_b[..., :3]).mean() > 0.2
    od = oracle.decode(b, want_dump=True)
    check_u8(inside[..., :3], NU.reference_pixels(od, w, h, RAMP, seeds=(0, 1))[:H - 100, :W - 40], "second layer")
