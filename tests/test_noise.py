"""Synthetic noise without a GPU: the numpy reference of the rules ("Noise: rules restated, not pinned") against the
known answers of their text, the reference's XYB -> u8 conversion against the oracle's own pixels, and what the host parser accepts and
refuses."""
import numpy as np
import pytest

import layer_util as LU
import noise_util as NU
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth

# the plain streams the GPU tests add noise to: (w, h, encoder arguments)
STREAMS = [(600, 400, dict()), (257, 300, dict(distance=4.0)), (333, 257, dict(gaborish=False, epf_iters=0)),
           (300, 280, dict(distance=4.0, epf_iters=3))]


def test_generator_known_answers():
    s0, s1 = NU.seed_state(0, 0, 0, 0)
    first = NU.batches(np.array(s0, np.uint64), np.array(s1, np.uint64), 1)[0]
    assert [int(v) for v in first[:4]] == [0xf63b9b5e, 0xc4415072, 0xfe79a97e, 0x9043044d]
    p = NU.group_planes(0, 0, 0, 0, 256, 64)
    assert p.dtype == np.float32 and p.shape == (3, 64, 256)
    assert [int(v) for v in p[0, 0, :4].view(np.uint32)] == [1073421773, 1071784104, 1073691860, 1070080386]
    assert [int(v) for v in NU.group_planes(0, 0, 256, 0, 16, 1)[0, 0, :2].view(np.uint32)] == [1068963656, 1065418508]
    assert p.min() >= 1.0 and p.max() < 2.0
    assert abs(float(p.mean()) - 1.4996) < 5e-4 and abs(float(p.std()) - 0.2894) < 5e-4


def test_frame_planes_are_filled_group_by_group():
    """Every 256 x 256 group on its own: the unused tail of a row's last batch is dropped, plane 0 first, rows in order."""
    R = NU.random_planes(600, 400)
    assert (R[:, :256, :256] == NU.group_planes(0, 0, 0, 0, 256, 256)).all()
    assert (R[:, 256:, 512:] == NU.group_planes(0, 0, 512, 256, 88, 144)).all()
    wide = NU.group_planes(0, 0, 512, 256, 96, 144)   # same six batches per row
    assert (R[:, 256:, 512:] == wide[:, :, :88]).all()
    assert not (R[:, :144, :88] == R[:, 256:, 512:]).any(axis=(1, 2)).all()
    assert (NU.random_planes(5, 3, 0, 1) != NU.random_planes(5, 3)).any()


def test_convolution_is_zero_mean_and_mirrors_the_edge():
    R = NU.random_planes(40, 9)
    N = NU.convolve(R)
    assert abs(N.mean()) < 0.02 and 0.2 < N.std() < 0.3
    flat = NU.convolve(np.full((3, 7, 6), 1.5, np.float32))   # weights sum to zero, also across the mirrored edge
    assert np.abs(flat).max() < 1e-12
    one = NU.convolve(NU.random_planes(1, 1))
    assert np.abs(one).max() < 1e-12


@pytest.mark.parametrize("w,h,kw", STREAMS)
def test_reference_conversion_matches_the_oracle(oracle, w, h, kw):
    """XYB -> u8 of the numpy reference on the oracle's filtered planes against the oracle's pixels: the reference alone stays well
    inside the cap of the GPU tests (1 LSB on at most 0.2 % of the samples)."""
    cs = oracle.encode(synth(w, h, 3), container=False, **kw)
    od = oracle.decode(cs, want_dump=True)
    got = NU.to_samples(NU.xyb_to_srgb(NU.planes_of(od, w, h)), np.uint8)
    d = np.abs(got.astype(int) - od.pixels[..., :3].astype(int))
    share = float((d > 0).mean())
    print("%dx%d %s: max %d LSB, %.5f %% of samples differ" % (w, h, kw, d.max(), 100 * share))
    assert d.max() <= 1 and share <= 0.002


def test_zero_strength_leaves_the_planes_alone(oracle):
    cs = oracle.encode(synth(64, 48, 5), container=False)
    od = oracle.decode(cs, want_dump=True)
    xyb = NU.planes_of(od, 64, 48)
    N = NU.convolve(NU.random_planes(64, 48))
    assert (NU.add_noise(xyb, N, [0] * 8) == xyb.astype(np.float64)).all()
    assert np.abs(NU.add_noise(xyb, N, [1023] * 8) - xyb).max() > 0.1


@pytest.mark.parametrize("w,h,passes", [(40, 30, 1), (300, 280, 1), (300, 280, 3)])
def test_parser_accepts_noise_frames(oracle, w, h, passes):
    cs = oracle.encode(synth(w, h, 7), container=False, num_passes=passes)
    status, _, msg = api.parse_check(NU.noisy(cs, [64] * 8, passes))
    assert status == "Ok", msg
    assert api.parse_check(cs)[0] == "Ok"


def test_parser_accepts_noise_on_replace_layers(oracle):
    a = oracle.encode(synth(120, 90, 1), container=False)
    b = oracle.encode(synth(50, 40, 2), container=False)
    data = LU.layered(a, [LU.Layer(a, crop=False), LU.Layer(NU.with_noise(b, [100] * 8), x0=20, y0=10, flags=1)])
    status, _, msg = api.parse_check(data)
    assert status == "Ok", msg


def test_refusals_keep_their_messages(oracle):
    lossy = oracle.encode(synth(40, 30, 7), container=False)
    lossless = oracle.encode(synth(40, 30, 7), container=False, lossless=True)
    # noise on a Modular frame
    status, _, msg = api.parse_check(LU.layered(lossless, [LU.Layer(lossless, crop=False, flags=1)]))
    assert status == "DecodeError" and "noise on Modular frames is not supported yet" in msg, msg
    # a parameter block that ends with the section: five bytes in a section of five bytes
    info, h, end = LU.frame_of(lossy)
    cut = NU.with_noise(lossy, None, param_bytes=b"\x55" * 5)
    cinfo, _, cend = LU.frame_of(cut)
    r = LU.BitReader(cut, cend)
    r.b()
    r.pos = (r.pos + 7) // 8 * 8
    first = r.u32(*NU.TOC)
    data_at = (r.pos + 7) // 8
    w = LU.BitWriter()
    w.raw(LU._bits_of(cut, cinfo.frame_start * 8, cend))
    w.b(False)
    w.align()
    w.u32(5, *NU.TOC)
    w.align()
    short = cut[:cinfo.frame_start] + w.tobytes() + cut[data_at:data_at + 5]
    assert first > 5
    status, _, msg = api.parse_check(LU.layered(lossy, [LU.Layer(short, crop=False, flags=1)]))
    assert status == "DecodeError" and "truncated noise parameters" in msg, msg
    # splines keep the combined message
    status, _, msg = api.parse_check(LU.layered(lossy, [LU.Layer(lossy, crop=False, flags=16)]))
    assert status == "DecodeError" and "noise / patches / splines are not supported yet" in msg, msg
