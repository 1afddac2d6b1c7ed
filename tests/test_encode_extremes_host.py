"""The preconditions of tests/test_gpu_encode_extremes.py, proved with the CPU oracle alone: each hostile picture of extremes_util.py
really produces the extreme it is there for (quantised HF values in the thousands, a densely filled 64x64 varblock, a group with nearly
every coefficient non-zero, frames with next to no HF, values at the int16 clamp), so that a later change of a picture cannot make a GPU
case vacuous.  These are conditions on the inputs, not measurements of the product: if one fails, change the picture, not the bound."""
import numpy as np
import pytest

import extremes_util as X


def max_abs_q(dump, channels=(0, 1, 2)):
    return max(int(np.abs(dump.planes["qcoef"][c]).max()) for c in channels)


def test_pictures_are_reproducible_and_read_only():
    for name in X.EIGHT_BIT + X.FLOATS:
        px = X.picture(name)
        assert not px.flags.writeable and px.dtype == (np.float32 if name in X.FLOATS else np.uint8)
    assert X.picture("noise").shape == (40, 72, 3) and X.picture("dense64").shape == (136, 200, 3)
    assert X.picture("full-group").shape == (264, 264, 4) and X.picture("hdr-step").shape == (40, 40, 3)
    assert set(np.unique(X.picture("bw-noise")).tolist()) == {0, 255} and X.coded(X.picture("bw-noise")).shape[2] == 1
    assert set(np.unique(X.picture("dense64")).tolist()) == {99, 100, 101}
    assert X.picture("hdr-noise").max() > 63 and X.picture("hdr-noise").min() >= 0 and X.picture("hdr-step").max() == 1000.0
    assert (X.picture("full-group")[..., 3] != 255).any()          # the alpha channel is coded
    assert X.coded(X.picture("red")).shape[2] == 3 and X.coded(X.picture("white")).shape[2] == 1


def test_a_black_white_edge_at_distance_0_05_quantises_into_the_thousands(oracle):
    d = X.oracle_dump("step8", 0.05, 1)
    q = int(np.abs(d.planes["qcoef"][1]).max())
    print("step8, distance 0.05, 8x8 only: max |qcoef Y| = %d" % q)
    assert q >= 2000                                               # measured 3084


def test_flat_noise_at_distance_0_05_fills_a_64x64_varblock(oracle):
    d = X.oracle_dump("dense64", 0.05, 0)
    s = d.planes["strategy"].reshape(d.h8, d.w8)
    nz = (X.by_cell(d.planes["qcoef"][1], d.h8, d.w8) != 0).sum(1).reshape(d.h8, d.w8)
    counts = [int(nz[by:by + 8, bx:bx + 8].sum()) for by, bx in zip(*np.nonzero(s == (0x80 | 18)))]
    print("dense64, distance 0.05: %d DCT64x64 varblocks, non-zero Y coefficients %s" % (len(counts), sorted(counts)))
    assert counts and max(counts) >= 3000                          # measured: 6 blocks, the densest with 3336 of 4096


def test_rgba_noise_at_distance_0_05_leaves_nearly_every_coefficient_non_zero(oracle):
    d = X.oracle_dump("full-group", 0.05, 0)
    share = sum(int((d.planes["qcoef"][c] != 0).sum()) for c in range(3)) / sum(d.planes["qcoef"][c].size for c in range(3))
    size = len(X.oracle_stream("full-group", 0.05, 0))
    print("full-group, distance 0.05: %.4f of all coefficients non-zero, %d bytes" % (share, size))
    assert share >= 0.95 and size >= 250000                        # measured 0.972, 287,503 bytes
    assert np.array_equal(d.pixels[..., 3], X.picture("full-group")[..., 3])


@pytest.mark.parametrize("mode", [1, 0], ids=["8x8", "default"])
def test_single_colours_and_distance_25_leave_next_to_no_hf(oracle, mode):
    worst = {}
    for name in X.EIGHT_BIT:
        for dist in X.DISTANCES:
            if name in X.SINGLE_COLOUR or dist == 25.0:
                worst[(name, dist)] = max_abs_q(X.oracle_dump(name, dist, mode))
    print(worst)
    assert max(worst.values()) <= 6, worst                         # measured: noise pictures 1 to 3, step8 6
    assert all(worst[(name, dist)] == 0 for name in X.SINGLE_COLOUR for dist in X.DISTANCES)


def test_a_float_step_of_1000_reaches_the_int16_clamp_and_decodes(oracle):
    """Without the clamp (oracle/jxo_enc.cc, DESIGN section 2 "Quantiser") this picture quantises to |Y| = 804376."""
    d = X.oracle_dump("hdr-step", 0.05, 0)
    assert max_abs_q(d) == 32767
    assert d.pixels.dtype == np.float32 and d.pixels.shape == (40, 40, 3) and np.isfinite(d.pixels).all()


def test_float_noise_up_to_64_stays_below_the_clamp_but_far_above_8_bit_input(oracle):
    d = X.oracle_dump("hdr-noise", 0.05, 0)
    q = max_abs_q(d)
    print("hdr-noise, distance 0.05: max |qcoef| = %d" % q)
    assert 4000 <= q < 32767                                       # measured: X 4036, Y 13912, B 5082
