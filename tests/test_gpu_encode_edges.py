"""GPU tests of the lossy encoder at tiny and edge-sized frames (sizes and pictures: encode_edges_util.py; what they rest on, shown on
the oracle alone: test_encode_edges_host.py).  The kernels of csrc/encode_kernels.hip branch on the frame's extent - replicated
padding, shapes rejected at the frame's edge, cells outside the frame inside a 64 x 64 region, groups and LF groups one cell or one
sample wide - and a whole-image PSNR does not see a wrong last column of cells.  Here every file is held to the oracle's encoder on
the same pixels plane by plane, and its decode to the source over the band where an edge fault would show.

No bound is new: |delta| <= 1 and the shares of test_quantised_data_matches_the_oracle_encoder, the oracle encoder's PSNR minus 0.5 dB
of test_save_image_round_trip_rgba (over the edge band), 1 LSB / 48 steps / 1e-3 / 2e-3 between the two decoders, |delta| <= 1 per
fitted map value (test_gpu_cfl_fit.py), bytes equal between the routes; planes and frames of fewer than 1000 values fall under the
small-frame rule of DESIGN.md section 7.  Every figure is printed before it is asserted."""
import functools
import math

import numpy as np
import pytest
import torch

import distance_util as DU
import encode_edges_util as E
import noise_util as NU
from pdn_jpegxl_amd import api
from test_gpu_parity import MAX_FRAC_DIFF

pytestmark = pytest.mark.gpu

EFFORT_IDS = ["fast", "squares", "default"]


@functools.lru_cache(maxsize=None)
def product_file(case, effort):
    """SaveImage's file of a picture at distance 1: saved once, shared."""
    return api.save_image(E.bgra_of(E.picture(case)), distance=1.0, effort=effort)


@functools.lru_cache(maxsize=None)
def product_dump(case, effort):
    import oracle_lib
    return oracle_lib.decode(product_file(case, effort), want_dump=True)


@pytest.fixture(scope="module")
def encoder():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the product path has no CPU fallback")
    enc = api.Encoder(0)
    yield enc
    enc.close()


def tie_of(case, effort):
    t = E.TIES.get(case + (effort,))
    return None if t is None else t[:2]


def raw(a):
    """The bytes of the samples: floats are compared by bit pattern."""
    return np.ascontiguousarray(a).view(np.uint8)


def band_check(od, src, theirs, what, bits=None):
    """The oracle's decode `od` of the product's file against the source over the edge band, beside the oracle's decode `theirs` of its
    own encoder's file: at least its PSNR minus 0.5 dB."""
    ours_db, theirs_db = E.db_of_rms(E.band_rms(od, src, bits)), E.db_of_rms(E.band_rms(theirs, src, bits))
    print("%s: band PSNR %.3f dB, oracle encoder %.3f dB (%+.3f)" % (what, ours_db, theirs_db, ours_db - theirs_db))
    assert math.isfinite(ours_db) and ours_db >= theirs_db - 0.5, (what, ours_db, theirs_db)


def decoders_agree(data, od, what, kind="u8", nch=4):
    """api.load_image of the product's file against the oracle's decode `od`: 1 LSB on at most 0.2 % of the samples (fewer than 1000
    samples: max(1, ceil(0.002 n)) of them) for 8-bit files, 48 steps of 16 bits, 1e-3 for binary32, 2e-3 for binary16; alpha equal."""
    got = api.load_image(data).pixels
    assert got.shape == od.shape and got.dtype == od.dtype, (what, got.shape, od.shape)
    ncol = nch - 1 if nch in (2, 4) else nch
    if kind in ("f16", "f32"):
        d = np.abs(got[..., :ncol].astype(np.float64) - od[..., :ncol].astype(np.float64))
        print("%s: max |product - oracle| = %.3g" % (what, d.max()))
        assert d.max() < (1e-3 if kind == "f32" else 2e-3), (what, float(d.max()))
    else:
        d = np.abs(got[..., :ncol].astype(np.int64) - od[..., :ncol].astype(np.int64))
        print("%s: max |product - oracle| = %d on %d of %d samples" % (what, d.max(), (d > 0).sum(), d.size))
        if kind == "u16":
            assert d.max() <= 48, (what, int(d.max()))
        else:
            n = d.size
            assert d.max() <= 1 and (d > 0).sum() <= (max(1, math.ceil(MAX_FRAC_DIFF * n)) if n < 1000 else MAX_FRAC_DIFF * n), (what, int(d.max()), int((d > 0).sum()))
    if nch in (2, 4):
        assert np.array_equal(raw(got[..., -1]), raw(od[..., -1])), what


# ---------------------------------------------------------------- 1. stage parity with the oracle's encoder
@pytest.mark.parametrize("effort,mode", E.EFFORTS, ids=EFFORT_IDS)
@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_quantised_data_matches_the_oracle_encoder(oracle, case, effort, mode):
    """Strategies, quant field, quantised LF and HF of SaveImage's file against the oracle encoder's file of the same pixels.  Effort 3:
    every strategy equal; efforts 5 and 7 on frames of fewer than 1000 cells: every strategy equal (E.TIES names the exceptions)."""
    what = "%s effort %d" % (E.case_id(case), effort)
    E.compare_planes(product_dump(case, effort), E.oracle_dump(case, mode), effort, what, tie_of(case, effort))


# ---------------------------------------------------------------- 2. the edge band
@pytest.mark.parametrize("effort,mode", E.EFFORTS, ids=EFFORT_IDS)
@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_edge_band_and_both_decoders(oracle, case, effort, mode):
    """The last 8 columns and rows (the whole of a frame of fewer than 1000 samples) of the oracle's decode of the product's file are
    as close to the source as those of the oracle encoder's file, less 0.5 dB; alpha is exact; the product reads its file as the oracle."""
    name, w, h = case
    src = E.picture(case)
    what = "%s effort %d" % (E.case_id(case), effort)
    data = product_file(case, effort)
    assert data[:12] == bytes([0, 0, 0, 0xC]) + b"JXL \r\n\x87\n"
    od = product_dump(case, effort).pixels
    assert od.shape == (h, w, 4) and np.array_equal(od[..., 3], src[..., 3]), what
    band_check(od, src, E.oracle_dump(case, mode).pixels, what)
    decoders_agree(data, od, what)


# ---------------------------------------------------------------- 3. the other input forms
def unscale(px16, bits):
    """16-bit output samples of a `bits`-bit stream -> the coded integers (tests/test_gpu_save_pixels.py)."""
    if bits == 16:
        return px16
    return np.round(px16.astype(np.float64) * ((1 << bits) - 1) / 65535.0).astype(np.uint16)


@pytest.mark.parametrize("effort,mode", E.EFFORTS, ids=EFFORT_IDS)
@pytest.mark.parametrize("size", E.DEEP_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("form", list(E.DEEP_FORMS))
def test_other_input_forms(oracle, form, size, effort, mode):
    """jxlhip_save_pixels on 10- and 16-bit integers, binary16, binary32 (one in Rec2020 PQ), gray, gray + alpha and opaque RGB of
    the same content: the checks of 1 and 2 against the oracle's encoder with the matching options."""
    w, h = size
    kind, bits, nch, colour, ocolour = E.DEEP_FORMS[form]
    px, kw, okw = E.deep_picture(form, w, h)
    what = "%s %dx%d effort %d" % (form, w, h, effort)
    data = api.save_pixels(px, distance=1.0, effort=effort, **kw)
    a = oracle.decode(data, want_dump=True)
    b = E.oracle_deep_dump(form, w, h, mode)
    E.compare_planes(a, b, effort, what)
    od = a.pixels
    assert od.shape == px.shape and od.dtype == (np.uint16 if kind == "u16" else px.dtype), what
    if nch in (2, 4):   # alpha is exact: integers by value, floats by bit pattern
        if kind == "u16":
            assert np.array_equal(unscale(od[..., -1], bits), px[..., -1]), what
        else:
            assert np.array_equal(raw(od[..., -1]), raw(px[..., -1])), what
    band_check(od, px, b.pixels, what, bits or None)
    decoders_agree(data, od, what, kind, nch)
    if colour != "Srgb":
        assert api.load_image(data).known_profile == colour


# ---------------------------------------------------------------- 4. fitted chroma-from-luma maps at partial tiles
@pytest.mark.parametrize("effort,mode", E.EFFORTS, ids=EFFORT_IDS)
@pytest.mark.parametrize("size", E.CFL_SIZES, ids=lambda s: "%dx%d" % s)
def test_fitted_maps_at_partial_tiles(oracle, size, effort, mode):
    """The maps of a save with the fit on against the oracle's fit of the same pixels: |delta| <= 1 in every tile at effort 3, at
    efforts 5 and 7 in every tile whose cells agree in strategy and raw quant value.  The tile at the right edge (one cell wide from
    65 x 63 on) holds cells outside the frame: what the kernel keeps of the dequantised Y there must not enter its sums."""
    w, h = size
    case = ("ramp_tex", w, h)
    img = E.picture(case)
    what = "cfl %dx%d effort %d" % (w, h, effort)
    data = api.save_pixels(img, distance=1.0, effort=effort, cfl=True)
    assert api.save_pixels(img, distance=1.0, effort=effort, cfl=True) == data     # the fit's sums are reduced in a fixed order
    ours = oracle.decode(data, want_dump=True)
    theirs = E.oracle_dump(case, mode, True)
    (ox, ob), (tx, tb) = E.maps_of(ours), E.maps_of(theirs)
    assert ox.shape == tx.shape == ((h + 63) // 64, (w + 63) // 64)
    assert tx[0, -1] != 0 or tb[0, -1] != 0, what      # the oracle's fit of the edge tile is not all zero (also test_encode_edges_host.py)
    assert tx[-1, 0] != 0 or tb[-1, 0] != 0, what
    ok = E.tiles_that_agree(ours, theirs)
    if effort == 3:
        assert (ours.planes["strategy"] == theirs.planes["strategy"]).all()
        ok[:] = True
    dx, db = np.abs(ox - tx), np.abs(ob - tb)
    print("%s: %d of %d tiles compared, max |delta| ytox %d ytob %d, %d of %d map values differ; edge tile ours (%d, %d) oracle (%d, %d)" %
          (what, ok.sum(), ok.size, dx[ok].max() if ok.any() else 0, db[ok].max() if ok.any() else 0, (dx[ok] > 0).sum() + (db[ok] > 0).sum(), 2 * ok.sum(),
           ox[0, -1], ob[0, -1], tx[0, -1], tb[0, -1]))
    assert ok.any(), what
    assert dx[ok].max() <= 1 and db[ok].max() <= 1, what
    od = ours.pixels
    assert od.shape == img.shape and np.array_equal(od[..., 3], img[..., 3]), what
    band_check(od, img, theirs.pixels, what)
    decoders_agree(data, od, what)


# ---------------------------------------------------------------- 5. routes that must agree byte for byte
def device_item(px, **kw):
    host = np.array(px, order="C")   # (a writable copy: the pictures are read-only)
    return api.EncodeItem.from_tensor(torch.from_numpy(host).cuda(), **kw)


def test_batch_of_every_case_writes_the_bytes_of_save_pixels(encoder):
    """All ramp_tex cases of point 1 (20 sizes x efforts 3 / 5 / 7) in one batch, in the table's order and in reverse; save_pixels
    on 8-bit RGBA in turn writes SaveImage's file."""
    specs = [(("ramp_tex", w, h), effort) for w, h in E.SIZES for effort, _ in E.EFFORTS]
    want = [api.save_pixels(E.picture(case), distance=1.0, effort=effort) for case, effort in specs]
    for (case, effort), f in zip(specs, want):
        assert f == product_file(case, effort), (case, effort)
    items = [device_item(E.picture(case), distance=1.0, effort=effort) for case, effort in specs]
    for order in (slice(None), slice(None, None, -1)):
        got = encoder.encode_batch(items[order])
        for (case, effort), g, f in zip(specs[order], got, want[order]):
            assert g == f, (case, effort, len(g or b""), len(f))


def test_batch_with_group_counts_1_9_9_side_by_side(encoder):
    cases = [("ramp_tex", 1, 1), ("ramp_tex", 2049, 9), ("ramp_tex", 9, 2049)]
    assert [((w + 255) // 256) * ((h + 255) // 256) for _, w, h in cases] == [1, 9, 9]
    for effort, _ in E.EFFORTS:
        got = encoder.encode_batch([device_item(E.picture(c), distance=1.0, effort=effort) for c in cases])
        for c, g in zip(cases, got):
            assert g == product_file(c, effort), (c, effort)


@pytest.mark.parametrize("size", E.LOOP_SIZES, ids=lambda s: "%dx%d" % s)
def test_effort_8_never_leaves_more_cells_over_the_target_than_effort_7(oracle, size):
    """test_never_more_cells_over_the_target_than_effort_7 of test_gpu_effort_loop.py on a picture that is neither flat nor whole cells:
    the float64 twin of the distance map on the oracle's decode of both files, and the loop's own counts."""
    w, h = size
    case = ("ramp_tex", w, h)
    img = E.picture(case)
    orig = DU.srgb8_to_xyb(img[..., :3])
    cells, figures = {}, {}
    for effort in (7, 8):
        data = api.save_image(E.bgra_of(img), distance=1.0, effort=effort)
        figures[effort] = api.last_save_distances()
        od = oracle.decode(data, want_dump=True)
        assert od.pixels.shape == img.shape and np.array_equal(od.pixels[..., 3], img[..., 3])
        decoders_agree(data, od.pixels, "%dx%d effort %d" % (w, h, effort))
        cells[effort] = DU.cell_distances(orig, NU.planes_of(od, w, h))
    tau = DU.target_of(cells[7])
    over = {e: DU.cells_over(cells[e], tau) for e in (7, 8)}
    f = figures[8]
    print("%dx%d: cells over tau = %.5f: %s; the loop's counts: first %d, emitted %d" % (w, h, tau, over, f["cells_over_target_first"], f["cells_over_target_emitted"]))
    assert figures[7]["evaluations"] == 0 and f["evaluations"] == 3
    assert f["cells"].size == ((w + 7) // 8) * ((h + 7) // 8)
    assert over[8] <= over[7], over
    assert f["cells_over_target_emitted"] <= f["cells_over_target_first"]
