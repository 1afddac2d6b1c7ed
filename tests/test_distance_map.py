"""The distance map's rules ("Distance map: rules of this project") on the CPU: properties of the float64 numpy twin
that the GPU kernels are compared with (tests/test_gpu_effort_loop.py), and the figures the design was measured with."""
import numpy as np
import pytest

import distance_util as DU
import noise_util as NU
from pdn_jpegxl_amd.synth import synth


def planes(h, w, seed):
    """XYB-like planes: smooth ramps plus a little texture, in the value range of real pictures."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([0.01 * np.cos(xx / 7.0), 0.4 + 0.2 * np.sin(yy / 9.0 + xx / 13.0), 0.35 + 0.1 * np.cos(yy / 5.0)])
    return base + 0.002 * rng.standard_normal((3, h, w))


def test_identical_pictures_have_distance_zero():
    o = planes(20, 27, 1)
    assert (DU.cell_distances(o, o) == 0).all()
    img = synth(40, 24, 2)
    assert (DU.distance_map(img, img) == 0).all()


def test_distance_is_linear_in_the_error():
    o = planes(33, 41, 3)
    e = 0.004 * np.random.default_rng(4).standard_normal(o.shape)
    one = DU.cell_distances(o, o + e)
    two = DU.cell_distances(o, o + 2 * e)
    assert one.min() > 0
    np.testing.assert_allclose(two, 2 * one, rtol=1e-12)


@pytest.mark.parametrize("w,h", [(1, 1), (2, 3), (7, 5), (9, 9)])
@pytest.mark.parametrize("offset", [0.01, -0.003])
def test_constant_offset_in_y_reads_as_its_size_in_every_cell(w, h, offset):
    """A constant error is all low band whatever the frame size: the blur's mirror has to repeat until the index is inside (frames
    narrower than the reach of 2, and of 4 for the nested blur)."""
    o = planes(h, w, 5)
    r = o.copy()
    r[1] += offset
    t = DU.cell_distances(o, r)
    assert t.shape == ((h + 7) // 8, (w + 7) // 8)
    np.testing.assert_allclose(t, DU.K * abs(offset), rtol=1e-9)


def test_reflect_repeats_until_inside():
    assert [DU.reflect(v, 1) for v in range(-4, 5)] == [0] * 9
    assert [DU.reflect(v, 2) for v in range(-4, 6)] == [0, 1, 1, 0, 0, 1, 1, 0, 0, 1]
    assert [DU.reflect(v, 5) for v in (-2, -1, 0, 4, 5, 6)] == [1, 0, 0, 4, 4, 3]


def test_texture_masks_a_fine_error_but_not_a_coarse_one():
    h, w = 32, 32
    rng = np.random.default_rng(6)
    flat = np.stack([np.zeros((h, w)), np.full((h, w), 0.5), np.full((h, w), 0.4)])
    textured = flat.copy()
    textured[1] += 0.05 * rng.standard_normal((h, w))
    fine = np.zeros((3, h, w))
    fine[1] = 0.004 * ((np.indices((h, w)).sum(0) & 1) * 2 - 1)   # a checkerboard: all in the high band
    t_flat = DU.cell_distances(flat, flat + fine)
    t_text = DU.cell_distances(textured, textured + fine)
    assert (t_text < 0.5 * t_flat).all()
    coarse = np.zeros((3, h, w))
    coarse[1] = 0.004                                               # all in the low band: masking does not touch it
    np.testing.assert_allclose(DU.cell_distances(textured, textured + coarse), DU.cell_distances(flat, flat + coarse), rtol=1e-9)


def test_channel_weights():
    o = planes(16, 16, 7)
    for c in range(3):
        r = o.copy()
        r[c] += 0.002
        np.testing.assert_allclose(DU.cell_distances(o, r), DU.K * DU.S[c] * 0.002, rtol=1e-9)


def test_forward_xyb_inverts_the_decoders_colour_transform():
    img = synth(48, 40, 8)[..., :3]
    back = NU.xyb_to_srgb(DU.srgb8_to_xyb(img)) * 255.0
    assert np.abs(back - img).max() < 1e-6


def test_target_and_counts():
    cells = np.arange(11, dtype=np.float64)[::-1].reshape(1, 11)
    assert DU.target_of(cells) == 9.0 and DU.cells_over(cells, 9.0) == 1      # rank floor(0.9 * 10) = 9 of 0..10
    assert DU.target_of(np.array([[3.0]])) == 3.0 and DU.cells_over(np.array([[3.0]]), 3.0) == 0


def test_design_figures_of_the_open_loop_encoder(oracle):
    """DESIGN.md §4.10 was measured with these constants on the oracle's encoder (the suite pins it to the GPU encoder's quantised
    data): cells of synth(512, 384, 7) at distance 1.0 have median 0.00413 and 90th percentile 0.00625."""
    img = synth(512, 384, 7)
    od = oracle.decode(oracle.encode(img, distance=1.0), want_dump=True)
    cells = DU.cell_distances(DU.srgb8_to_xyb(img[..., :3]), NU.planes_of(od, 512, 384))
    assert cells.shape == (48, 64)
    assert "%.3g" % np.median(cells) == "0.00413", np.median(cells)
    assert "%.3g" % np.percentile(cells, 90) == "0.00625", np.percentile(cells, 90)
