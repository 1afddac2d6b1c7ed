"""GPU parity with side information that varies: chroma-from-luma maps per tile, EPF sharpness per cell, custom
chroma-from-luma parameters, LF dequantisation factors, qm scales, Gaborish weights, the three EPF parameter bundles and custom quant
biases, written by the oracle's writer (oracle/jxo_codec.h: SideInfo).

The bar is test_gpu_parity.py's, unchanged: integer planes bit-exact (now with maps that are not constant, which are also checked
against the numpy restatement of the writer's formulas), stage taps within TOL_LF / TOL_XYB, u8 samples within MAX_LSB on at most
MAX_FRAC_DIFF of the samples."""
import numpy as np
import pytest

import downscale_util as DU
import side_info_util as S
from gpu_helpers import gpu_decode
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth
from test_gpu_downscale import check_u8
from test_gpu_parity import check_pixels, run_case

pytestmark = pytest.mark.gpu

W, H = 264, 200   # 5 x 4 tiles with ragged right and bottom edges, 2 x 1 groups: the tile column 4 lies in the second group


def layout_of(img, layout):
    return np.ascontiguousarray({"rgba": img, "rgb": img[..., :3], "gray": img[..., 1:2]}[layout])


def general_kernel(dec, data):
    """The same stream through filter_stream_kernel instead of filter_stream_pairs_kernel."""
    try:
        assert dec.set_option("no_stream_pairs", 1)
        return gpu_decode(dec, [data])[0]
    finally:
        dec.set_option("no_stream_pairs", 0)


# ---------------------------------------------------------------- chroma-from-luma maps
@pytest.mark.parametrize("layout", ["rgba", "rgb", "gray"])
@pytest.mark.parametrize("strategy_mode", [0, 2])
@pytest.mark.parametrize("mode", ["fitted", "formula"])
def test_cfl_maps(gpu_decoder, oracle, mode, strategy_mode, layout):
    """recon_tile_kernel with factors that differ from tile to tile, -128 and 127 among them (formula), and with the factors an
    encoder would choose (fitted).  Gray frames are coded as XYB too and carry both maps; the decoder applies them to X and B, which
    the gray sample (the green of the XYB -> RGB matrix) reads, so the same bar holds there.  (A gray source has X = 0 and B = Y, so
    its FITTED maps are within a step or two of zero and its picture is nearly the plain stream's: only the formula maps are
    required to move a gray picture.)"""
    src = layout_of(synth(W, H, 1), layout)
    data, od = run_case(gpu_decoder, oracle, src, strategy_mode=strategy_mode, seed=3, side_info=dict(cfl=mode, seed=5))
    if mode == "formula":
        S.check_formula_planes(od, W, H, 5, sharpness=False)
    else:
        assert od.planes["ytox"].any() or od.planes["ytob"].any()
    if (mode, layout) != ("fitted", "gray"):
        plain = oracle.decode(oracle.encode(src, strategy_mode=strategy_mode, seed=3)).pixels
        assert (od.pixels != plain).mean() > 0.01


@pytest.mark.parametrize("s", [21, 22, 23, 24, 25, 26])
def test_cfl_maps_under_varblocks_larger_than_a_tile(gpu_decoder, oracle, s):
    """dequant_kernel (the path of varblocks of 128 and 256 points a side) takes the factors of the tile that holds the varblock's
    FIRST cell for every coefficient of the varblock, whichever tile the coefficient's footprint position lies in."""
    data, od = run_case(gpu_decoder, oracle, synth(520, 300, 3), strategy_mode=3, fixed_strategy=s, side_info=dict(cfl="formula", seed=11))
    S.check_formula_planes(od, 520, 300, 11, sharpness=False)
    first = od.planes["strategy"][(od.planes["strategy"] & 0x80) != 0] & 0x7F
    assert (first == s).any()


# ---------------------------------------------------------------- sharpness
@pytest.mark.parametrize("size", [(122, 20), (257, 301), (58, 70)])
@pytest.mark.parametrize("epf_iters,distance", [(1, 1.0), (2, 2.5), (3, 4.5)])
@pytest.mark.parametrize("sharpness", ["formula", 0, 7])
def test_sharpness(gpu_decoder, oracle, sharpness, epf_iters, distance, size):
    """cell_sigma_kernel reads every entry of the sharpness table, and the filter kernels see a sigma that changes from cell to cell:
    the stage kernels (taps), the streaming kernels of both forms (122 x 20: pairs kernel with a strip edge; 257 x 301: odd width,
    general kernel), against the oracle and against each other."""
    w, h = size
    img = synth(w, h, 17 + epf_iters)
    data, od = run_case(gpu_decoder, oracle, img, distance=distance, epf_iters=epf_iters, side_info=dict(sharpness=sharpness, seed=7))
    assert od.epf_iters == epf_iters
    if sharpness == "formula":
        S.check_formula_planes(od, w, h, 7, cfl=False)
    else:
        assert (od.planes["sharpness"] == sharpness).all()
    streamed = gpu_decode(gpu_decoder, [data])[0]
    check_pixels(streamed, od.pixels)
    staged = gpu_decode(gpu_decoder, [data], taps=True)[0]
    d = np.abs(streamed.astype(np.int32) - staged.astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 2e-3
    assert np.array_equal(streamed, general_kernel(gpu_decoder, data))
    plain = oracle.decode(oracle.encode(img, distance=distance, epf_iters=epf_iters)).pixels
    assert (od.pixels != plain).any()


# ---------------------------------------------------------------- geometry: LF groups, one-section frames
@pytest.mark.parametrize("size", [(2056, 16), (16, 2056)])
def test_two_lf_groups(gpu_decoder, oracle, size):
    """The second LF group is one cell and one tile wide (or high): its maps are 1 x 1 and 1 x 2 planes with a stride of their own."""
    w, h = size
    data, od = run_case(gpu_decoder, oracle, synth(w, h, 4), distance=2.5, side_info=dict(cfl="formula", sharpness="formula", seed=13))
    S.check_formula_planes(od, w, h, 13)


@pytest.mark.parametrize("layout", ["rgba", "rgb"])
@pytest.mark.parametrize("size", [(200, 120), (8, 8), (1, 1)])
def test_one_section_frames_with_every_knob(gpu_decoder, oracle, size, layout):
    w, h = size
    src = layout_of(synth(w, h, 41), layout)
    data, od = run_case(gpu_decoder, oracle, src, distance=2.5, side_info=S.EVERYTHING)
    S.check_formula_planes(od, w, h, S.EVERYTHING["seed"])
    got = api.load_image(data)      # the call the reference's host makes
    check_pixels(got.pixels, od.pixels)


# ---------------------------------------------------------------- other ways to write the same maps
@pytest.mark.parametrize("passes", [2, 3])
def test_progressive_passes_with_formula_maps(gpu_decoder, oracle, passes):
    img = synth(W, H, 75 + passes)
    side = dict(cfl="formula", sharpness="formula", seed=17)
    data, od = run_case(gpu_decoder, oracle, img, num_passes=passes, side_info=side)
    S.check_formula_planes(od, W, H, 17)
    one = oracle.decode(oracle.encode(img, side_info=side)).pixels
    assert (od.pixels == one).all()
    check_pixels(gpu_decode(gpu_decoder, [data])[0], one)


@pytest.mark.parametrize("opts", [dict(prefix_codes=True), dict(lz77=True), dict(prefix_codes=True, lz77=True)], ids=["prefix", "lz77", "prefix+lz77"])
@pytest.mark.parametrize("size", [(W, H), (200, 120)])
def test_maps_through_the_general_symbol_reader(gpu_decoder, oracle, opts, size):
    """Prefix codes / LZ77: the metadata stream's maps are decoded sample by sample (several groups, and a one-section frame)."""
    w, h = size
    data, od = run_case(gpu_decoder, oracle, synth(w, h, 93), distance=2.5, side_info=dict(cfl="formula", sharpness="formula", seed=19), **opts)
    S.check_formula_planes(od, w, h, 19)


# ---------------------------------------------------------------- header knobs
HEADER_KNOBS = sorted(k for k in S.KNOBS if not k.startswith(("cfl-fitted", "cfl-formula", "sharp-formula", "sharp-0", "sharp-7")))


@pytest.mark.parametrize("distance", [2.5, 4.5])
@pytest.mark.parametrize("knob", HEADER_KNOBS)
def test_header_knobs(gpu_decoder, oracle, knob, distance):
    """Custom chroma-from-luma parameters (every branch of color_factor), LF factors, qm scales ((0, 7) and (7, 0) included), Gaborish
    weights per channel, sharpness table, EPF channel scales and sigma bundle, quant biases: one by one and all together, with two
    (distance 2.5) and three (4.5) EPF iterations."""
    img = synth(W, H, 1)
    data, od = run_case(gpu_decoder, oracle, img, distance=distance, side_info=S.KNOBS[knob])
    check_pixels(gpu_decode(gpu_decoder, [data])[0], od.pixels)      # the streaming kernels (run_case decodes stage by stage)
    plain = oracle.decode(oracle.encode(img, distance=distance)).pixels
    assert (od.pixels != plain).mean() > 0.01


# ---------------------------------------------------------------- bands, batches, reduced size
@pytest.mark.parametrize("world", [2, 3])
def test_bands_with_formula_maps(gpu_decoder, oracle, world):
    """Each band bit-identical to the same rows of the whole frame: the maps of the halo rows reach the band's filters."""
    from pdn_jpegxl_amd.distributed import decode_frame_band
    w, h = 300, 600
    data = oracle.encode(synth(w, h, 31), distance=4.5, side_info=dict(cfl="formula", sharpness="formula", seed=23))
    od = oracle.decode(data)
    whole = gpu_decode(gpu_decoder, [data])[0]
    check_pixels(whole, od.pixels)
    rows = 0
    for rank in range(world):
        band, (y0, y1) = decode_frame_band(gpu_decoder, data, rank, world)
        assert np.array_equal(band.cpu().numpy().reshape(y1 - y0, w, 4), whole[y0:y1]), (rank, y0, y1)
        rows += y1 - y0
    assert rows == h


def test_one_batch_of_frames_with_different_knobs(gpu_decoder, oracle):
    """No parameter leaks from one image of a batch to the next: every output equals that frame decoded alone, byte for byte."""
    sides = [S.EVERYTHING, S.KNOBS["cfl-params-cf256-zero-maps"], None, S.KNOBS["sharp-lut"], S.KNOBS["quant-biases"], S.KNOBS["epf-sigma"]]
    sizes = [(W, H), (200, 120), (W, H), (257, 301), (122, 20), (W, H)]
    files = [oracle.encode(synth(w, h, 50 + i), distance=2.5, side_info=s) for i, (s, (w, h)) in enumerate(zip(sides, sizes))]
    alone = [gpu_decode(gpu_decoder, [f])[0] for f in files]
    for order in (list(range(6)), [2, 0, 5, 1, 4, 3]):
        together = gpu_decode(gpu_decoder, [files[i] for i in order])
        for i, out in zip(order, together):
            assert np.array_equal(out, alone[i]), (order, i)
    for f, a in zip(files, alone):
        check_pixels(a, oracle.decode(f).pixels)


@pytest.mark.parametrize("knob", ["cfl-params-cf84-zero-maps", "cfl-params-cf256-zero-maps", "cfl-params-cf11-zero-maps", "cfl-params-cf1000-zero-maps",
                                  "lf-factors", "all-compensated"])
@pytest.mark.parametrize("size", [(W, H), (23, 9)])
def test_reduced_size_decode_with_custom_lf_parameters(gpu_decoder, oracle, knob, size):
    """downscale = 8 hands out the LF image: custom LF factors, base correlations, ytox_lf and ytob_lf, against the float64 reference of
    the colour rule on the oracle's LF dump (test_gpu_downscale.py).  Opaque frames.  That reference converts with the default opsin
    matrix, so the custom transform data of `all-compensated` (quant biases, which no LF sample reads) is left out here."""
    w, h = size
    side = dict(S.KNOBS[knob])
    side.pop("quant_biases", None)
    img = synth(w, h, 3)[..., :3]
    data = oracle.encode(img, distance=1.0, side_info=side)
    od = oracle.decode(data, want_dump=True)
    got = DU.decode_reduced(gpu_decoder, data)
    assert got.shape == ((h + 7) // 8, (w + 7) // 8, 3) and got.dtype == np.uint8
    check_u8(got, DU.reference_colour(od), "%s %dx%d" % (knob, w, h))
    # the writer compensates, so the picture is the plain stream's up to quantisation; the quantised LF is not
    plain = oracle.decode(oracle.encode(img, distance=1.0), want_dump=True)
    assert any((od.planes["lf_quant"][c] != plain.planes["lf_quant"][c]).any() for c in range(3))


# ---------------------------------------------------------------- refusal
@pytest.mark.parametrize("size", [(W, H), (40, 24)])
@pytest.mark.parametrize("what", ["sharpness", "cfl"])
def test_out_of_range_maps_are_refused(gpu_decoder, oracle, what, size):
    """One sharpness value of 8 / one chroma-from-luma value of 128: DecodeError through LoadImage and through the batch call, never
    status Ok (several groups / a one-section frame)."""
    import torch
    data = oracle.encode(synth(size[0], size[1], 2), side_info=dict(refuse=what))
    with pytest.raises(oracle.OracleError):
        oracle.decode(data)
    with pytest.raises(api.FormatError) as e:
        api.load_image(data)
    assert e.value.status == "DecodeError"
    info = api.peek(data)
    out = torch.zeros(info.width * info.height * info.num_channels, dtype=torch.uint8, device="cuda")
    st = gpu_decoder.decode_batch([data], [out.data_ptr()], None, raise_on_error=False)
    assert st == [api.DECODER_STATUS.index("DecodeError")], st
    # the same picture without the switch decodes
    check_pixels(gpu_decode(gpu_decoder, [oracle.encode(synth(size[0], size[1], 2))])[0], oracle.decode(oracle.encode(synth(size[0], size[1], 2))).pixels)
