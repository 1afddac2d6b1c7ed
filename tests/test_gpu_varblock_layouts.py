"""Varblock layouts that no encoder writes, on the GPU: blocks that do not start on a multiple of their size, that straddle 64x64 tiles
and chroma-from-luma tiles, rows of free cells cut into runs by what hangs from above - and the sequences a decoder must refuse.

The streams come from the oracle's writer (`varblocks=` / `varblock_sequence=` of oracle_lib.encode; case table and the numpy
restatement of the placement rule: tests/varblock_util.py; CPU side: tests/test_varblock_layouts.py).  The bar is test_gpu_parity's:
block metadata and quantised coefficients exact, float stages within TOL_LF / TOL_XYB, 8-bit samples within 1 LSB on at most
MAX_FRAC_DIFF of them.  `query_generic_tiles` says how many 64x64 tiles recon_tile_kernel left to the generic kernels; the expected
number comes from the layout alone (varblock_util.generic_tiles)."""
import numpy as np
import pytest

from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth
from gpu_helpers import gpu_decode
from test_gpu_parity import check_pixels, run_case
import downscale_util as DU
import varblock_util as V

pytestmark = pytest.mark.gpu

FILL = 0xA5


def stream(oracle, case, **kw):
    return oracle.encode(V.smooth(case.w, case.h), distance=1.0, varblocks=case.blocks, **kw)


def listed(dec):
    return dec.set_option("query_generic_tiles", 0)


def check_case(dec, oracle, case, tiles=None, **kw):
    """The production decode (streaming filters) with its count of generic tiles, then the staged decode with every tap."""
    img = V.smooth(case.w, case.h)
    kw = dict(dict(distance=1.0, varblocks=case.blocks), **kw)
    data = oracle.encode(img, **kw)
    plain = gpu_decode(dec, [data])[0]
    assert listed(dec) == (len(V.generic_tiles(case.plane)) if tiles is None else tiles)
    check_pixels(plain, oracle.decode(data).pixels)
    _, od = run_case(dec, oracle, img, **kw)
    assert np.array_equal(od.planes["strategy"].reshape(case.h8, case.w8), case.plane)   # (the stream holds the layout the case names)
    return data, plain


# ---------------------------------------------------------------- valid layouts
@pytest.mark.parametrize("case", V.CASES, ids=repr)
def test_layout(gpu_decoder, oracle, case):
    """Every case of the table; the count of generic tiles first (aligned-pairs: 0, recon_tile_kernel did all of it; big-128: the nine
    tiles the block touches - tests/test_varblock_layouts.py::test_named_cases pins what the layout side derives)."""
    check_case(gpu_decoder, oracle, case)


# ---------------------------------------------------------------- the entropy side of the same layouts
@pytest.mark.parametrize("name", ["small-shifts", "split-rows"])
def test_lane_mappings_agree(gpu_decoder, oracle, name):
    data = stream(oracle, V.BY_NAME[name])
    a = gpu_decode(gpu_decoder, [data], lane_stride=1)[0]
    b = gpu_decode(gpu_decoder, [data], lane_stride=64)[0]
    assert np.array_equal(a, b)
    check_pixels(a, oracle.decode(data).pixels)


@pytest.mark.parametrize("opts", [dict(prefix_codes=True, lz77=True), dict(custom_orders=True), dict(num_passes=2), dict(custom_quant_tables=True)],
                         ids=["prefix+lz77", "orders", "two-passes", "own-tables"])
@pytest.mark.parametrize("name", ["small-shifts", "split-rows"])
def test_entropy_variants(gpu_decoder, oracle, name, opts):
    case = V.BY_NAME[name]
    every_tile = ((case.w8 + 7) // 8) * ((case.h8 + 7) // 8)     # a progressive frame goes generic as a whole
    check_case(gpu_decoder, oracle, case, tiles=every_tile if "num_passes" in opts else None, **opts)


@pytest.mark.parametrize("name", ["small-shifts", "tile-corner-64"])
def test_chroma_from_luma_of_the_origin_tile(gpu_decoder, oracle, name):
    """Maps that change from tile to tile and reach -128 and 127: a block's factors are those of the tile that holds its origin, for
    every cell of it, also those in the next tile."""
    case = V.BY_NAME[name]
    assert V.census(case.plane)["crosses_cfl_tile"]
    data, _ = check_case(gpu_decoder, oracle, case, side_info=dict(cfl="formula", seed=3))
    od = oracle.decode(data, want_dump=True)
    assert od.planes["ytox"].min() == -128 and od.planes["ytox"].max() == 127 and len(set(od.planes["ytob"].tolist())) > 1


# ---------------------------------------------------------------- other routes
def lone(dec, data):
    return gpu_decode(dec, [data])[0]


def test_mixed_batch(gpu_decoder, oracle):
    """The list of generic tiles and its length are per image: an aligned frame, big-128 and small-shifts in one batch each decode to
    the bytes of their lone decodes."""
    files = [oracle.encode(synth(272, 200, 12), distance=1.0), stream(oracle, V.BY_NAME["big-128"]), stream(oracle, V.BY_NAME["small-shifts"])]
    alone = [lone(gpu_decoder, f) for f in files]
    counts = []
    for f in files:
        lone(gpu_decoder, f)
        counts.append(listed(gpu_decoder))
    together = gpu_decode(gpu_decoder, files)
    assert listed(gpu_decoder) == sum(counts)
    for a, b in zip(alone, together):
        assert np.array_equal(a, b)


def test_band_decode(gpu_decoder, oracle):
    """big-128 has two group rows; each rank's band equals the rows of the whole decode."""
    from pdn_jpegxl_amd.distributed import decode_frame_band
    case = V.BY_NAME["big-128"]
    data = stream(oracle, case)
    whole = lone(gpu_decoder, data)
    rows = 0
    for rank in range(2):
        band, (y0, y1) = decode_frame_band(gpu_decoder, data, rank, 2)
        assert np.array_equal(band.cpu().numpy().reshape(y1 - y0, case.w, 4), whole[y0:y1]), rank
        rows += y1 - y0
    assert rows == case.h


def test_reduced_size_decode(gpu_decoder, oracle):
    """The 1:8 decode reads the LF image only, but the placement still runs on the misaligned layout."""
    from test_gpu_downscale import check_u8
    case = V.BY_NAME["odd-64s"]
    data = stream(oracle, case)
    od = oracle.decode(data, want_dump=True)
    gpu_decoder.set_option("debug_taps", 0)
    got = DU.decode_reduced(gpu_decoder, data)
    assert got.shape == (case.h8, case.w8, 4)
    check_u8(got[..., :3], DU.reference_colour(od), "odd-64s at 1:8")
    assert (got[..., 3] == 255).all()


# ---------------------------------------------------------------- layouts a decoder must refuse
def bad_stream(oracle, item):
    name, w, h, seq, reason = item
    return oracle.encode(V.smooth(w, h), distance=1.0, varblock_sequence=seq)


def decode_filled(dec, files):
    """One batch into buffers filled with FILL; returns (statuses, host copies of the buffers)."""
    import torch
    dec.set_option("debug_taps", 0)
    dec.set_option("lane_stride", 0)
    infos = [api.peek(f) for f in files]
    outs = [torch.full((i.width * i.height * i.num_channels,), FILL, dtype=torch.uint8, device="cuda") for i in infos]
    torch.cuda.synchronize()
    st = dec.decode_batch(files, [o.data_ptr() for o in outs], None, raise_on_error=False)
    return st, [o.cpu().numpy().reshape(i.height, i.width, i.num_channels) for o, i in zip(outs, infos)]


@pytest.fixture(scope="module")
def neighbours(oracle):
    """Two valid misaligned streams and their decodes by a decoder that has seen nothing else."""
    good = [stream(oracle, V.BY_NAME["tile-corner-64"]), stream(oracle, V.BY_NAME["odd-pairs"])]
    fresh = api.Decoder(0)
    try:
        return good, [lone(fresh, g) for g in good]
    finally:
        fresh.close()


@pytest.mark.parametrize("item", V.INVALID, ids=[i[0] for i in V.INVALID])
def test_invalid_sequences_are_refused(gpu_decoder, oracle, neighbours, item):
    """An error status, never status Ok with cells nobody placed.  The host's parse has nothing to object to (the block metadata is
    decoded on the GPU); LoadImage and the batch call end in DecodeError, the neighbours in the batch decode as they do alone, the
    refused image's buffer keeps its fill, and the same decoder then decodes a valid misaligned layout to the bytes a fresh one gives."""
    data = bad_stream(oracle, item)
    with pytest.raises(oracle.OracleError) as e:
        oracle.decode(data)
    assert item[4] in str(e.value)
    assert api.parse_check(data)[0] == "Ok"
    with pytest.raises(api.FormatError) as e:
        api.load_image(data)
    assert e.value.status == "DecodeError"
    # refused by the placement, before the HF sections (which hold the tokens of another layout) could fail for reasons of their own
    assert "invalid-varblock-layout" in str(e.value), str(e.value)
    good, alone = neighbours
    st, outs = decode_filled(gpu_decoder, [good[0], data, good[1]])
    assert st == [0, api.DECODER_STATUS.index("DecodeError"), 0], st
    assert np.array_equal(outs[0], alone[0]) and np.array_equal(outs[2], alone[1])
    assert np.array_equal(lone(gpu_decoder, good[1]), alone[1])
    assert (outs[1] == FILL).all(), "the refused image's buffer was written to"
