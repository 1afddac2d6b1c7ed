"""GPU tests of lossy saves and lossy decodes at the ends of the distance range (0.05 and 25; 0.1 beside them) on the hostile pictures
of extremes_util.py: quantised HF values in the thousands, densely filled 64x64 varblocks, a group whose coefficients are nearly all
non-zero, frames with no HF at all, float samples far above 1.0 (the int16 clamp of the quantiser).  tests/test_encode_extremes_host.py
proves on the CPU that the pictures produce these extremes.

Every bound is one the suite already holds elsewhere: 1 LSB between the product's and the oracle's decode (test_gpu_encode.py), the
oracle encoder's PSNR minus 0.5 dB (test_save_image_round_trip_rgba; no absolute floor - the oracle itself reaches 21 dB on noise, DESIGN
section 2 "Quantiser"), |delta| <= 1 on quantised data with the flip shares of test_quantised_data_matches_the_oracle_encoder scaled by
max(1, 1 / distance), test_gpu_parity.py's stage tolerances, test_float_samples_lossy's 1e-3 for binary32."""
import functools

import numpy as np
import pytest

from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth
from gpu_helpers import compare_stages, gpu_decode
from save_pixels_util import psnr_nominal
from test_gpu_parity import check_pixels, check_report
import extremes_util as X

pytestmark = pytest.mark.gpu

TOL_F32 = 1e-3     # test_gpu_formats.py: test_float_samples_lossy, binary32
SYNTH = "synth"    # a 200 x 136 synth() picture beside the hostile ones (RGBA, soft alpha)


def source(name):
    return synth(200, 136, 7) if name == SYNTH else X.picture(name)


@functools.lru_cache(maxsize=None)
def product_file(name, distance, effort):
    """The product's file of a picture: SaveImage for 8-bit pictures, jxlhip_save_pixels for the float ones.  Saved once, shared."""
    px = source(name)
    if px.dtype == np.float32:
        return api.save_pixels(px, distance=distance, effort=effort)
    return api.save_image(X.bgra_surface(px), distance=distance, effort=effort)


@functools.lru_cache(maxsize=None)
def oracle_file(name, distance, mode):
    import oracle_lib
    if name == SYNTH:
        return oracle_lib.encode(source(name), distance=distance, strategy_mode=mode)
    return X.oracle_stream(name, distance, mode)


def colour_of(px):
    return px[..., :px.shape[2] - 1] if px.shape[2] in (2, 4) else px


def both_decodes_agree(oracle, data, what, relative=False):
    """oracle.decode accepts the file and api.load_image agrees with it: 8-bit within 1 LSB, binary32 within TOL_F32 - absolute, or with
    `relative` times max(1, largest |sample| of the oracle's decode).  TOL_F32 was set for samples on the nominal scale [0, 1], where it
    is 8400 float32 ulps of the largest sample; the two decoders differ by float32 summation order, an error relative to the magnitude
    (an ulp of 1000 is 6.1e-5: the absolute bound there would be 16 ulps), so the relative form holds a frame whose samples reach M
    to the same number of ulps of M.  Returns both decodes."""
    od = oracle.decode(data).pixels
    got = api.load_image(data).pixels
    assert got.shape == od.shape and got.dtype == od.dtype, what
    if od.dtype == np.float32:
        d = np.abs(got.astype(np.float64) - od.astype(np.float64))
        largest = float(np.abs(od).max())
        print("%s: max |product - oracle| = %.3g (largest sample %.4g)" % (what, d.max(), largest))
        assert d.max() < TOL_F32 * (max(1.0, largest) if relative else 1.0), (what, float(d.max()), largest)
    else:
        d = np.abs(got.astype(int) - od.astype(int))
        print("%s: max |product - oracle| = %d LSB on %.4f of the samples" % (what, d.max(), (d > 0).mean()))
        assert d.max() <= 1, (what, int(d.max()))
    return od, got


def fidelity(decoded, src):
    if src.dtype == np.float32:
        return psnr_nominal(colour_of(decoded).astype(np.float64), colour_of(src).astype(np.float64))
    return X.psnr8(colour_of(decoded), colour_of(src))


# ---------------------------------------------------------------- a. round trip
@pytest.mark.parametrize("effort", [3, 7])
@pytest.mark.parametrize("distance", X.DISTANCES)
@pytest.mark.parametrize("name", X.EIGHT_BIT + X.FLOATS)
def test_round_trip(oracle, name, distance, effort):
    src = X.picture(name)
    data = product_file(name, distance, effort)
    what = "%s d=%g effort %d" % (name, distance, effort)
    # binary32: relative to the largest sample (64 and 1000 here; measured on the nominal scale at distances 0.1 and 25: 1.04e-3 to
    # 1.22e-3, 10 ulps of 1025); at distance 0.05 case f below also holds both float pictures to the absolute TOL_F32
    od, got = both_decodes_agree(oracle, data, what, relative=True)
    coded = src if src.dtype == np.float32 else X.coded(src)
    assert od.shape == coded.shape
    if name == "full-group":
        assert np.array_equal(od[..., 3], src[..., 3]) and np.array_equal(got[..., 3], src[..., 3])   # alpha is lossless
    ours = fidelity(od, coded)
    theirs = fidelity(oracle.decode(oracle_file(name, distance, X.MODE_OF_EFFORT[effort])).pixels, coded)   # the oracle at exactly 25 too
    print("%s: %d bytes, PSNR %.2f dB, oracle encoder %.2f dB" % (what, len(data), ours, theirs))
    assert ours >= theirs - 0.5, (what, ours, theirs)


# ---------------------------------------------------------------- b. quantised data against the oracle's encoder
LIMIT_HF, LIMIT_HF_B, LIMIT_LF = 0.004, 0.015, 0.01   # test_quantised_data_matches_the_oracle_encoder, at distance 1


@pytest.mark.parametrize("effort,mode", [(3, 1), (5, 4), (7, 0)], ids=["fast", "squares", "default"])
@pytest.mark.parametrize("distance", [0.05, 0.1])
@pytest.mark.parametrize("name", ["noise", "bw-noise", "step8", "blue-yellow8", "dense64", SYNTH])
def test_quantised_data_matches_the_oracle_encoder_at_small_distances(oracle, name, distance, effort, mode):
    """The comparison of test_gpu_encode.py.  The hard rule is unchanged (|delta| <= 1 wherever strategy and quant field agree); the
    share of values that may differ by that one step is the distance-1 limit times max(1, 1 / distance): a value flips when the two
    float32 paths differ by more than its margin to the rounding boundary, and that margin, in quantiser steps, shrinks in proportion
    to the step, which shrinks in proportion to the distance.  A 1 % scale error in a basis row or a weight moves a value of 3000 by
    30 steps here; at distance 1 it moves no value by more than the one step the rule allows."""
    k = max(1.0, 1.0 / distance)
    a = oracle.decode(product_file(name, distance, effort), want_dump=True)
    b = oracle.decode(oracle_file(name, distance, mode), want_dump=True)
    what = "%s d=%g effort %d" % (name, distance, effort)
    sa, sb = a.planes["strategy"], b.planes["strategy"]
    assert sa.shape == sb.shape and (a.h8, a.w8) == (b.h8, b.w8)
    same = sa == sb
    print("%s: strategy agreement %.5f" % (what, same.mean()))
    assert same.mean() > 0.995, what
    if mode == 1:
        assert same.all() and ((sa & 0x7F) == 0).all()
    rq = (a.planes["raw_quant"] != b.planes["raw_quant"]) | ~same
    print("%s: raw quant disagreement %.5f" % (what, rq.mean()))
    assert rq.mean() < LIMIT_LF * k, what
    for c in range(3):
        d = np.abs(a.planes["lf_quant"][c].astype(int) - b.planes["lf_quant"][c].astype(int))[same]
        print("%s: LF %s max %d share %.5f (largest value %d)" % (what, "XYB"[c], d.max(), (d > 0).mean(), np.abs(b.planes["lf_quant"][c]).max()))
        assert d.max() <= 1 and (d > 0).mean() < LIMIT_LF * k, (what, c, int(d.max()), float((d > 0).mean()))
    cells_ok = ~rq.reshape(-1)
    assert cells_ok.any()
    for c in range(3):
        qa = X.by_cell(a.planes["qcoef"][c], a.h8, a.w8)[cells_ok].astype(int)
        qb = X.by_cell(b.planes["qcoef"][c], b.h8, b.w8)[cells_ok].astype(int)
        d = np.abs(qa - qb)
        print("%s: HF %s max %d share %.5f (largest value %d, non-zero %.3f)" % (what, "XYB"[c], d.max(), (d > 0).mean(), np.abs(qb).max(), (qb != 0).mean()))
        assert d.max() <= 1 and (d > 0).mean() < (LIMIT_HF_B if c == 2 else LIMIT_HF) * k, (what, c, int(d.max()), float((d > 0).mean()))


# ---------------------------------------------------------------- c. decode parity on oracle-written extremes
@pytest.mark.parametrize("name,distance", [("step8", 0.05), ("step8", 25.0), ("noise", 0.05), ("noise", 25.0), ("dense64", 0.05), ("dense64", 25.0),
                                           ("full-group", 0.05)])
def test_decode_parity_on_oracle_written_extremes(gpu_decoder, oracle, name, distance):
    data = oracle_file(name, distance, 0)
    od = oracle.decode(data, want_dump=True)
    out = gpu_decode(gpu_decoder, [data], taps=True)[0]
    check_report(compare_stages(gpu_decoder, 0, od))
    check_pixels(out, od.pixels)


def test_dense_large_blocks_in_a_mixed_batch_under_every_lane_mapping(gpu_decoder, oracle):
    """dense64's 64x64 varblocks hold over 3000 non-zero coefficients each: decoded with one section per wavefront and in the per-lane
    form, beside a synth() frame, as test_batch_and_lane_mappings_agree does for sparse large blocks."""
    files = [oracle_file("dense64", 0.05, 0), oracle_file(SYNTH, 1.0, 0), oracle_file("dense64", 25.0, 0)]
    refs = [oracle.decode(f).pixels for f in files]
    base = None
    for stride in (64, 8, 1):
        outs = gpu_decode(gpu_decoder, files, lane_stride=stride)
        for o, r in zip(outs, refs):
            check_pixels(o, r)
        if base is None:
            base = outs
        else:
            for p, q in zip(base, outs):
                assert (p == q).all()   # the mapping of sections to lanes must not change a single bit


# ---------------------------------------------------------------- d. the clamps
def test_distances_outside_the_range_are_clamped_and_the_rate_follows_the_distance():
    surface = X.bgra_surface(X.picture("noise"))
    at = {d: product_file("noise", d, 7) for d in (0.05, 1.0, 25.0)}
    assert api.save_image(surface, distance=0.01, effort=7) == at[0.05]
    assert api.save_image(surface, distance=100.0, effort=7) == at[25.0]
    print("noise: %d / %d / %d bytes at distances 0.05 / 1 / 25" % (len(at[0.05]), len(at[1.0]), len(at[25.0])))
    assert len(at[0.05]) > len(at[1.0]) > len(at[25.0])


# ---------------------------------------------------------------- e. batch and effort tiers
def test_extremes_in_one_batch_write_the_bytes_of_save_pixels():
    import torch
    specs = [("full-group", 0.05), ("black", 25.0), ("dense64", 0.05)]
    items, want = [], []
    for name, distance in specs:
        px = X.picture(name)
        dev = torch.from_numpy(px.copy()).cuda()
        items.append(api.EncodeItem.from_tensor(dev, distance=distance, effort=7))
        want.append(api.save_pixels(px, distance=distance, effort=7))
    enc = api.Encoder(0)
    try:
        got = enc.encode_batch(items)
    finally:
        enc.close()
    for (name, distance), g, w in zip(specs, got, want):
        assert g == w, (name, distance, len(g or b""), len(w))
    assert len(want[0]) >= 250000   # full-group: nearly kAcTokCap tokens, the section's size in the TOC's 22-bit class


@pytest.mark.parametrize("name", ["step8", "hdr-noise"])
def test_effort_9_at_distance_0_05_decodes_on_both_sides(oracle, name):
    """The closed loop may raise a varblock's quant value to 4 x its base (dist_correct_kernel): values 4 x those of effort 7."""
    data = product_file(name, 0.05, 9)
    od, got = both_decodes_agree(oracle, data, "%s d=0.05 effort 9" % name)
    assert od.shape[:2] == X.picture(name).shape[:2]


# ---------------------------------------------------------------- f. float samples far above 1.0: the int16 clamp
@pytest.mark.parametrize("name", ["hdr-step", "hdr-noise"])
def test_float_samples_far_above_one_are_written_so_that_they_load(oracle, name):
    """enc_varblock_kernel clamps quantised HF values to +-32767, what hf_decode_kernel's int16 entries hold (it refuses wider values
    with its range error): without the clamp hdr-step's file (|Y| up to 804376) is one the product writes and then refuses to read."""
    data = product_file(name, 0.05, 7)
    both_decodes_agree(oracle, data, "%s d=0.05 effort 7" % name)
    a = oracle.decode(data, want_dump=True)
    b = X.oracle_dump(name, 0.05, 0)
    ours = [int(np.abs(a.planes["qcoef"][c]).max()) for c in range(3)]
    theirs = [int(np.abs(b.planes["qcoef"][c]).max()) for c in range(3)]
    print("%s: max |qcoef| X, Y, B = %s, oracle encoder %s" % (name, ours, theirs))
    if name == "hdr-step":
        assert max(ours) == 32767 and ours[1] == 32767 and theirs[1] == 32767     # the clamp is reached, on both sides
    else:
        assert 4000 <= max(ours) < 32767                                             # far above any 8-bit input, below the clamp
