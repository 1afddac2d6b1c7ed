"""The preconditions of tests/test_gpu_encode_edges.py, proved with the CPU oracle alone: at every size of encode_edges_util.py's
table, in each of the oracle encoder's strategy modes, the pictures are not flat, put non-zero HF coefficients into the varblocks at
the right and bottom edge, put 16-point and larger shapes there where the frame has room for them, and leave an error in the edge band
that a comparison can measure.  These are conditions on the inputs, not measurements of the product: if one fails, change the
picture, not the bound.  They keep the GPU tests from passing vacuously - synth() is a single colour at every size up to 7 x 7."""
import numpy as np
import pytest

import encode_edges_util as E

MODES = [1, 4, 0]


def test_pictures_are_reproducible_and_read_only():
    for case in E.CASES:
        name, w, h = case
        px = E.picture(case)
        assert px.shape == (h, w, 4) and px.dtype == np.uint8 and not px.flags.writeable, case
        assert px is E.picture(case)
        a = px[..., 3]
        assert not (a == 255).all() and not (a == 0).all(), case    # alpha is coded
        if w * h > 1:
            assert np.ptp(a) > 0, case                               # and varies
        assert not (px[..., 0] == px[..., 1]).all() and not (px[..., 1] == px[..., 2]).all(), case   # three colour channels are coded


def test_the_case_table():
    assert len(E.SIZES) == len(set(E.SIZES)) == 20 and max(max(s) for s in E.SIZES) == 2049
    assert E.SMOOTH_SIZES == E.SIZES and len(E.CASES) == 40 and set(E.DEEP_SIZES) | set(E.CFL_SIZES) | set(E.LOOP_SIZES) <= set(E.SIZES)
    assert len(E.TIES) <= 2


def test_ramp_tex_rises_to_the_last_column_and_row():
    """Without the texture every channel rises on every row to the last column and on every column to the last row, by more than a level a
    sample over the last nine; with it the last column and row stand above the ones eight before them."""
    for w, h in ((72, 72), (9, 2049), (2049, 9)):
        col, _, _ = E._ramps(w, h, E.RAMP_TEX_AMPS, 30.0, (230.0, 200.0, 170.0))
        assert (np.diff(col[:, -9:], axis=1) > 1).all() and (np.diff(col[-9:], axis=0) > 1).all()
        px = E.ramp_tex(w, h, 5).astype(int)
        assert (px[:, -1, :3].mean(0) > px[:, -8, :3].mean(0) + 6).all() and (px[-1, :, :3].mean(0) > px[-8, :, :3].mean(0) + 6).all()


@pytest.mark.parametrize("mode", MODES, ids=["mode1", "mode4", "mode0"])
@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_the_oracles_own_file(oracle, case, mode):
    name, w, h = case
    px = E.picture(case)
    d = E.oracle_dump(case, mode)
    # decodes, with the stated shape and exact alpha
    assert d.pixels.shape == (h, w, 4) and d.pixels.dtype == np.uint8, case
    assert np.array_equal(d.pixels[..., 3], px[..., 3]), case
    assert (d.w8, d.h8) == ((w + 7) // 8, (h + 7) // 8)
    st = d.planes["strategy"].reshape(d.h8, d.w8)
    # not flat
    if (w, h) == (1, 1):
        assert all(d.planes["lf_quant"][c].size == 1 for c in range(3)) and d.planes["lf_quant"][1][0] != 0   # one sample: its LF only
    else:
        assert all(np.ptp(px[..., c]) > 0 for c in range(3)), case
        nonzero = [int((d.planes["qcoef"][c] != 0).sum()) for c in range(3)]
        assert nonzero[1] > 0, (case, nonzero)
        if w >= 8 and h >= 8:   # at least one whole cell: HF in a varblock at the right edge and in one at the bottom edge, in Y
            col, row = E.edge_blocks_with_hf(d)
            assert col > 0 and row > 0, (case, col, row)
    # shapes at the edge
    first = st[st >= 0x80] & 0x7F
    if mode == 1:
        assert (first == 0).all()
    if name == "smooth_edge" and (w >= E.SMOOTH_FROM[0] and h >= E.SMOOTH_FROM[1] or max(w, h) > 2048):
        at_edge = set(np.unique(st[:, -1] & 0x7F).tolist()) | set(np.unique(st[-1] & 0x7F).tolist())
        if mode == 0:
            assert at_edge - {0}, (case, at_edge)
            assert at_edge & {4, 5, 6, 7, 10, 11}, (case, at_edge)
        elif mode == 4:
            assert set(first.tolist()) & {4, 5}, case
    # the band measure
    rms = E.band_rms(d.pixels, px)
    assert np.isfinite(rms) and rms > 0.3, (case, rms)


def test_rectangular_shapes_on_one_pixel_wide_frames(oracle):
    """On smooth_edge mode 0 covers a 1 x 9 frame's two cells with one 16 x 8 block and a 9 x 1 frame's with one 8 x 16 block: the second cell holds
    nothing but padding."""
    assert (E.oracle_dump(("smooth_edge", 1, 9), 0).planes["strategy"] & 0x7F).tolist() == [6, 6]
    assert (E.oracle_dump(("smooth_edge", 9, 1), 0).planes["strategy"] & 0x7F).tolist() == [7, 7]


def test_large_candidates_are_rejected_at_the_edge_of_127x129(oracle):
    """16 x 17 cells: a 32 x 32 block fits nowhere in the last cell row; the row holds 8 x 8 and 8 x 16 blocks only."""
    d = E.oracle_dump(("smooth_edge", 127, 129), 0)
    st = d.planes["strategy"].reshape(d.h8, d.w8)
    assert (d.w8, d.h8) == (16, 17) and set(np.unique(st[-1] & 0x7F).tolist()) <= {0, 7}
    assert (st[-1] & 0x7F == 7).any()


@pytest.mark.parametrize("form", list(E.DEEP_FORMS))
def test_the_other_input_forms(oracle, form):
    """The same content in every sample type: the oracle's file decodes to the type and shape, alpha exact, a few float samples above
    1.0, and the edge band's error is measurable."""
    kind, bits, nch, colour, ocolour = E.DEEP_FORMS[form]
    for w, h in E.DEEP_SIZES:
        px, kw, okw = E.deep_picture(form, w, h)
        assert px.shape == (h, w, nch) and not px.flags.writeable
        if kind in ("f16", "f32") and colour == "Srgb" and w * h > 2:
            above = (px[..., :min(nch, 3)].astype(np.float64) > 1.0).mean()
            assert 0 < above < 0.25, (form, w, h, above)
        d = E.oracle_deep_dump(form, w, h, 0)
        assert d.pixels.shape == px.shape and d.pixels.dtype == (np.uint16 if kind == "u16" else px.dtype)
        if nch in (2, 4):
            if kind == "u16":
                back = np.round(d.pixels[..., -1].astype(np.float64) * ((1 << bits) - 1) / 65535.0).astype(np.uint16)
                assert np.array_equal(back, px[..., -1]), (form, w, h)
            else:
                assert np.array_equal(d.pixels[..., -1], px[..., -1]), (form, w, h)
        assert any((d.planes["qcoef"][c] != 0).any() for c in range(3)), (form, w, h)
        rms = E.band_rms(d.pixels, px, bits or None)
        assert np.isfinite(rms) and rms > 0.3, (form, w, h, rms)


@pytest.mark.parametrize("size", E.CFL_SIZES, ids=lambda s: "%dx%d" % s)
def test_fitted_maps_of_the_partial_tiles_are_not_zero(oracle, size):
    """The oracle's fit on ramp_tex gives the tile at the right and at the bottom edge (one cell wide or deep at 65 x 63, 72 x 8 and
    257 x 255) map values that are not both zero: a fit that took in what lies outside the frame would show."""
    w, h = size
    for mode in MODES:
        d = E.oracle_dump(("ramp_tex", w, h), mode, True)
        ytox, ytob = E.maps_of(d)
        assert ytox.shape == ((d.h8 + 7) // 8, (d.w8 + 7) // 8)
        assert ytox[0, -1] != 0 or ytob[0, -1] != 0, (size, mode)
        assert ytox[-1, 0] != 0 or ytob[-1, 0] != 0, (size, mode)
