"""The entropy decoders on code forms the oracle's writer never chose on its own (tests/entropy_forms_util.py; held to the oracle and to
the streams' default forms on the CPU by tests/test_entropy_forms.py): HybridTail with every kind of configuration, one per code and
mixed per cluster; SlowGet with every special distance, plain distances, clamped and stream-starting copies, other thresholds and length
codes; alias tables from flat, reduced-precision and run-length histograms; context maps sent move-to-front.

The bar is bit-exact, nothing left out.  A lossless frame is its source and the oracle's pixels, in every launch shape.  A lossy frame
has the oracle's quantised LF, block metadata, quantised HF and alpha (compare_stages), and its bytes are those of the product's own
decode of the default stream of the same picture, shape by shape; pixels against the oracle keep test_gpu_parity's bounds.  Each case
first asserts, on the CPU, the launch plan it is built for (test_entropy_plan.plan_of), as test_gpu_global_tables does."""
import numpy as np
import pytest

import entropy_forms_util as EU
from gpu_helpers import compare_stages, gpu_decode
from pdn_jpegxl_amd import api
from test_entropy_plan import plan_of
from test_gpu_alpha_one_pass import decode as lane_path_decode
from test_gpu_ma_trees import batch, launch_shapes
from test_gpu_parity import check_pixels, check_report

pytestmark = pytest.mark.gpu

SHAPE_OPTS = {"default": dict(), "mod_lanes64": dict(mod_lanes64=True), "mod_lanes64 + no_direct": dict(mod_lanes64=True, no_direct=True)}


@pytest.fixture(scope="module")
def streams(oracle):
    """case id -> (source, file, the oracle's pixels), encoded and decoded once."""
    memo = {}

    def get(case):
        if case.id not in memo:
            data = case.encode(oracle)
            memo[case.id] = (case.picture(), data, oracle.decode(data).pixels)
        return memo[case.id]
    return get


def assert_plan(case, data):
    """What the case is built to reach, with exactly the options the decodes below set."""
    prefix = bool(case.enc.get("prefix_codes"))
    slow = prefix or "lz" in case.entropy
    for shape, opts in SHAPE_OPTS.items():
        P = plan_of([data], **opts)
        f = P["frames"][0]
        assert f["decoded"] and f["encoding"] == int(case.lossless) and f["mcode"][3] == int(prefix), (case.id, shape)
        for key, value in case.plan.items():
            assert P[key] == value, (case.id, shape, key, P[key])
        for key in ("mod_global", "lf_global", "hf_global", "alpha_global"):
            assert P[key] == case.plan.get(key, P[key] if not case.lossless and slow else 0), (case.id, shape, key)
        if case.lossless:
            assert P["mod_lanes"] == 1 if shape == "default" else P["mod_lanes"] in (8, 64), (case.id, shape, P["mod_lanes"])
            assert P["direct_mod"] == int(shape == "default"), (case.id, shape)
        else:
            assert (P["lane_stride"], P["lf_per_wave"], P["per_alpha_wg"]) == (64, 1, 1), (case.id, shape)   # one section per wavefront
            assert P["lean_mod"] == int(not slow and "lf_tree" not in case.enc), (case.id, shape)   # the lean form: plain ANS, the writer's own tree
    if not case.lossless:
        P = plan_of([data], lane_stride=2, no_direct=True)   # lane_path_decode's shape: HfBatchedLoop unless the code is a slow one
        assert (P["lane_stride"], P["per_alpha_wg"], P["global_direct"]) == (2, 32, 0), case.id


def check_lossless(dec, streams, cases, together):
    """Every case alone in the three launch shapes (together: as one batch in two) is its source and the oracle's pixels."""
    srcs, files = [streams(c)[0] for c in cases], [streams(c)[1] for c in cases]
    for c in cases:
        assert_plan(c, streams(c)[1])
        assert streams(c)[2].tobytes() == streams(c)[0].tobytes(), c.id
    got = launch_shapes(dec, files, together=together)
    assert set(got) == ({"default", "mod_lanes64"} if together else set(SHAPE_OPTS))
    bad = []
    for shape, outs in got.items():
        for c, g, s in zip(cases, outs, srcs):
            if not (g.dtype == s.dtype and g.shape == s.shape and g.tobytes() == s.tobytes()):
                bad.append("%s, %s: %d samples differ" % (c.id, shape, int((g != s).sum()) if g.shape == s.shape else -1))
    assert not bad, "; ".join(bad)
    return got["default"]


LOSSLESS = [c for c in EU.CASES if c.lossless and c.group != "lz-special"]
LOSSY = [c for c in EU.CASES if not c.lossless]


@pytest.mark.parametrize("case", LOSSLESS, ids=[c.id for c in LOSSLESS])
def test_lossless_frame_in_every_launch_shape(gpu_decoder, streams, case):
    src, data, _ = streams(case)
    check_lossless(gpu_decoder, streams, [case], together=False)
    one = api.load_image(data).pixels
    assert one.dtype == src.dtype and one.tobytes() == src.tobytes(), case.id


def test_every_special_distance_in_one_batch(gpu_decoder, oracle, streams):
    """The 120 rows of the table over 24 frames of 40 x 24, one decode_batch (tables per image), and each frame alone."""
    cases = EU.cases_of("lz-special")
    seen = set()
    for c in cases:
        c.encode(oracle)
        cen = oracle.entropy_census()
        seen |= {k for k in range(120) if cen["special"][k]}
    assert seen == set(range(120))
    check_lossless(gpu_decoder, streams, cases, together=True)
    check_lossless(gpu_decoder, streams, cases, together=False)


@pytest.fixture(scope="module")
def plain(gpu_decoder, oracle):
    """Per picture: the default stream of the same call, the product's decode of it in the shapes below, and its stage planes."""
    memo = {}

    def get(case):
        data = case.encode(oracle, entropy=False)
        if data not in memo:
            memo[data] = decode_shapes(gpu_decoder, data) + (stage_planes(gpu_decoder, data),)
        return memo[data]
    return get


def decode_shapes(dec, data):
    """(one section per wavefront, two lanes a section, the lane path with alpha in one pass, the lane path with int32 alpha residuals)"""
    return (batch(dec, [data])[0].tobytes(), batch(dec, [data], lane_stride=2)[0].tobytes(),
            lane_path_decode(dec, [data])[0][0].tobytes(), lane_path_decode(dec, [data], narrow_limit=0)[0][0].tobytes())


def stage_planes(dec, data=None):
    """The bit-exact planes of image 0 of the last decode with stage taps (of `data`, decoded here, when given)."""
    if data is not None:
        gpu_decode(dec, [data], taps=True)
    out = [dec.read_plane(0, "lf_quant", c).tobytes() for c in range(3)] + [dec.read_plane(0, "qcoef", c).tobytes() for c in range(3)]
    out += [dec.read_plane(0, n).tobytes() for n in ("cellinfo", "raw_quant", "sharpness", "ytox", "ytob", "alpha")]
    dec.set_option("debug_taps", 0)
    return out


@pytest.mark.parametrize("case", LOSSY, ids=[c.id for c in LOSSY])
def test_lossy_frame_against_the_oracle_and_its_default_stream(gpu_decoder, oracle, streams, plain, case):
    src, data, _ = streams(case)
    assert_plan(case, data)
    od = oracle.decode(data, want_dump=True)
    out = gpu_decode(gpu_decoder, [data], taps=True)[0]
    check_report(compare_stages(gpu_decoder, 0, od))
    check_pixels(out, od.pixels)
    planes = stage_planes(gpu_decoder)
    want = plain(case)
    assert planes == want[4], "a bit-exact plane differs from the decode of the default stream"
    got = decode_shapes(gpu_decoder, data)
    names = ("one section per wavefront", "lane_stride 2", "lane path", "lane path, alpha_narrow_limit 0")
    for name, g, w in zip(names, got, want[:4]):
        assert g == w, (case.id, name)
    assert np.array_equal(np.frombuffer(got[0], np.uint8).reshape(src.shape)[..., 3], src[..., 3])
    check_pixels(np.frombuffer(got[0], np.uint8).reshape(src.shape), od.pixels)


MIXED = ["cfg/mixed default", "cfg/632 prefix rows", "cfg-lossy/mixed 264", "cfg-lossy/632 prefix 64", "lz-special/file 00", "lz-clamp/2x64 index 17",
         "lz-misc/general, distance tail", "lz-lossy/general 64", "lz-zero-start/lossless", "lz-zero-start/lossy 264", "hist/flat lossy",
         "hist/rle lossless", "hist/mtf lossy", "cfg/000 16-bit noise grid"]


def test_mixed_batch_equals_each_file_alone(gpu_decoder, streams):
    """One case of every group in ONE decode_batch (ANS, prefix and LZ77 codes, lossless and lossy, side by side): byte-identical to
    each file's own batch."""
    by = {c.id: c for c in EU.CASES}
    cases = [by[name] for name in MIXED]
    assert {c.group for c in cases} == {c.group for c in EU.CASES}
    files = [streams(c)[1] for c in cases]
    together = batch(gpu_decoder, files)
    for c, f, t in zip(cases, files, together):
        alone = batch(gpu_decoder, [f])[0]
        assert alone.dtype == t.dtype and alone.tobytes() == t.tobytes(), c.id
        if c.lossless:
            assert t.tobytes() == streams(c)[0].tobytes(), c.id


def test_corrupt_streams_end_as_the_oracle_says(gpu_decoder, oracle):
    """Flipped bits in the first copy's length and distance, and a stream cut short: where the oracle reports an error the product
    reports one with a message (through slow_err, the range checks and the final-state check - no fault), and where the damaged stream
    is still a stream (extra bits are outside the ANS state) the product decodes the oracle's pixels, wrong as they are."""
    src, data, variants = EU.corrupt_variants(oracle)
    assert batch(gpu_decoder, [data])[0].tobytes() == src.tobytes()
    errors = 0
    for name, bad in variants:
        try:
            want = oracle.decode(bad).pixels
        except oracle.OracleError:
            want = None
        if want is None:
            errors += 1
            with pytest.raises(api.JxlError) as e:
                batch(gpu_decoder, [bad])
            assert len(str(e.value)) > len(e.value.status) + 2, (name, str(e.value))
        else:
            assert batch(gpu_decoder, [bad])[0].tobytes() == want.tobytes(), name
    assert errors >= 2
    assert batch(gpu_decoder, [data])[0].tobytes() == src.tobytes()   # the decoder is none the worse for it
