"""The entropy kernels with their tables in global memory (the kLds = false instantiations of lf_ans_kernel, alpha_ans_kernel,
modular_ans_kernel and hf_decode_kernel), reached the way real files reach them: an MA tree or a set of alias tables that does not fit
the launch's LDS (csrc/lds_layout.h: kLdsMax; csrc/entropy_plan.cc picks the form for a whole launch).

  * big trees: `big_tree` below, 4 901 .. 9 601 nodes of 16 bytes, through oracle.encode(tree= / alpha_tree= / lf_tree=)
  * wide codes: oracle.encode(wide_codes=True) writes the plain ANS codes with log_alpha 8 (2 KB of alias table per cluster) and keeps
    up to 255 used contexts apart: a hundred used leaves or the HF contexts of an ordinary picture are then enough

Which instantiation a launch runs cannot be observed from outside.  Every case therefore first asserts, on the CPU and with exactly the
options it then sets on the decoder, the plan fields it is built to reach (test_entropy_plan.plan_of); a case whose plan does not say
"global" fails there.  No environment knob is used.

Ground truth: a lossless frame is its source, bit for bit.  A tree or a code width changes the coding of a lossy frame and not its
content: alpha is the source's, the quantised LF and HF coefficients are the oracle's, and the bytes are those of the GPU's own decode
of the same picture written with the default tree / without the knob.  The only tolerances are those of test_gpu_parity (float stage
taps, u8 pixels against the oracle)."""
import numpy as np
import pytest

import downscale_util as DU
import ma_tree_util as M
from gpu_helpers import compare_stages, gpu_decode
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth, synth16
from test_entropy_plan import constants, layout, plan_of
from test_gpu_alpha_narrow import eligible_groups
from test_gpu_alpha_one_pass import decode as one_pass_decode
from test_gpu_ma_trees import batch, launch_shapes
from test_gpu_parity import check_pixels, check_report

pytestmark = pytest.mark.gpu

# launch_shapes' names -> the options it sets, as plan_of takes them
SHAPE_OPTS = {"default": dict(), "mod_lanes64": dict(mod_lanes64=True), "mod_lanes64 + no_direct": dict(mod_lanes64=True, no_direct=True)}


def big_tree(prop, n, forms, start=0):
    """A balanced tree of n thresholds around zero on one property: n + 1 leaves that cycle through `forms`, 2 n + 1 nodes."""
    leaf = M.Leaves(forms, start)
    return M.flatten(M.buckets(prop, list(range(-(n // 2), n - n // 2)), [leaf() for _ in range(n + 1)]))


def spread_tree(prop, n, step, forms):
    """n thresholds `step` apart around zero: the buckets a noise picture fills."""
    leaf = M.Leaves(forms)
    return M.buckets(prop, [step * (k - n // 2) for k in range(n)], [leaf() for _ in range(n + 1)])


def noise(w, h, nch, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, nch), dtype=np.uint8)


def rgb(w, h, seed):
    return np.ascontiguousarray(synth(w, h, seed)[..., :3])


def same_planes(a, b, names=("qcoef", "lf_quant", "strategy", "raw_quant")):
    for name in names:
        pa, pb = a.planes[name], b.planes[name]
        if isinstance(pa, list):
            assert all(np.array_equal(x, y) for x, y in zip(pa, pb)), name
        else:
            assert np.array_equal(pa, pb), name


# ================================================================ a. modular_ans_kernel<false>
def assert_mod_plan(files, shape, lanes, rb, wp):
    """The Modular launch of `files` under launch_shapes' shape `shape` keeps its tables in global memory, in the given lane shape."""
    opts = SHAPE_OPTS[shape]
    P = plan_of(files, **opts)
    assert all(f["decoded"] and f["encoding"] == 1 for f in P["frames"])
    assert P["mod_global"] == 1 and P["lds_mod"] > constants()["lds_max"], (shape, P["lds_mod"])
    assert (P["mod_lanes"], P["mod_rb"], P["mod_wp_lds"]) == (lanes[shape], rb, wp), (shape, P["mod_lanes"], P["mod_rb"], P["mod_wp_lds"])
    assert P["direct_mod"] == int(shape == "default")   # planned; the wrapper passes no scalar rows to the global form
    if opts.get("no_direct"):
        assert not P["global_direct"]
    return P


def check_lossless(dec, oracle, src, data, lanes, rb, wp):
    assert np.array_equal(oracle.decode(data).pixels, src)
    for shape in SHAPE_OPTS:
        assert_mod_plan([data], shape, lanes, rb, wp)
    one = api.load_image(data).pixels
    assert one.dtype == src.dtype and one.shape == src.shape
    assert one.tobytes() == src.tobytes(), "LoadImage: %d samples differ" % int((one != src).sum())
    got = launch_shapes(dec, [data])
    assert set(got) == set(SHAPE_OPTS)
    for shape, (g,) in got.items():
        assert g.dtype == src.dtype and g.shape == src.shape, shape
        bad = np.argwhere(g != src)
        assert g.tobytes() == src.tobytes(), "%s: %d samples differ, the first at (y, x, c) = %s" % (shape, len(bad), tuple(bad[0]) if len(bad) else ())


LANES_PLAIN = {"default": 1, "mod_lanes64": 64, "mod_lanes64 + no_direct": 64}
LANES_WP = {"default": 1, "mod_lanes64": 8, "mod_lanes64 + no_direct": 8}   # weighted-predictor state in LDS: eight sections per workgroup

# (id, picture, tree, encode options, lanes per shape, mod_rb, mod_wp_lds)
#   per-sample property, mixed predictors: the walk (ModularChannel<false>) with lanes == 1 and row buffers - no uniform shape there -
#     and with 64 lanes; one section (160x130) and several (257x200: global stream + pass groups; 400x380 gray: four groups)
#   property 2 alone, predictors 0 / 1 / 2 / 5: ClassifyChannel<false>, the row loops of DecodeChannelLane on global tables,
#     modular_finish_kernel behind them; no row buffers
#   weighted predictor on leaves and as property 15: its state in LDS beside the row buffers, lanes 1 and 8
#   Squeeze: 257x200 (residual channels in the pass groups) and 2100x33 (a channel of shift 3 wider than a group: LF-group streams too)
BIG = [
    ("p10 walk 160x130", lambda: rgb(160, 130, 1), lambda: big_tree(10, 2450, [5, 4, 7]), {}, LANES_PLAIN, 256, 0),
    ("p15 weighted 160x130", lambda: rgb(160, 130, 2), lambda: big_tree(15, 2450, [6, 5, 4, 7]), {}, LANES_WP, 256, 1),
    ("p10 walk 257x200", lambda: rgb(257, 200, 3), lambda: big_tree(10, 4800, [5, 4, 7]), {}, LANES_PLAIN, 256, 0),
    ("p2 static 257x200", lambda: rgb(257, 200, 4), lambda: big_tree(2, 4800, [0, 1, 2, 5]), {}, LANES_PLAIN, 0, 0),
    ("p15 weighted 257x200", lambda: rgb(257, 200, 5), lambda: big_tree(15, 4800, [6, 5, 4, 7]), {}, LANES_WP, 256, 1),
    ("p10 squeeze 257x200", lambda: rgb(257, 200, 6), lambda: big_tree(10, 4800, [5, 4, 7]), dict(lossless_squeeze=True), LANES_PLAIN, 256, 0),
    ("p10 squeeze 2100x33 gray", lambda: M.picture(2100, 33, 1, 5), lambda: big_tree(10, 2450, [5, 4, 7]), dict(lossless_squeeze=True), LANES_PLAIN, 256, 0),
    ("p10 walk 400x380 gray", lambda: M.picture(400, 380, 1, 7), lambda: big_tree(10, 4800, [5, 4, 7]), {}, LANES_PLAIN, 256, 0),
    ("p10 walk 160x130 16 bit", lambda: np.ascontiguousarray(synth16(160, 130, 8, 16)[..., :3]), lambda: big_tree(10, 2450, [5, 4, 7]), dict(bits=16), LANES_PLAIN, 256, 0),
]


@pytest.mark.parametrize("case", BIG, ids=[c[0] for c in BIG])
def test_lossless_frame_with_a_tree_too_big_for_lds(gpu_decoder, oracle, case):
    name, picture, tree, enc, lanes, rb, wp = case
    src = picture()
    data = oracle.encode(src, lossless=True, tree=tree(), **enc)
    f = plan_of([data])["frames"][0]
    assert 16 * f["tree_nodes"] > constants()["lds_max"] // 2 and f["mcode"][1] <= 7   # the tree, not the code, is what does not fit
    if "2100x33" in name:
        assert f["nlf"] == 2 and f["ng"] == 9
    check_lossless(gpu_decoder, oracle, src, data, lanes, rb, wp)


def test_one_big_tree_takes_the_whole_launch_to_global_tables(gpu_decoder, oracle):
    """A launch has one form: a frame with a 9 601-node tree beside ordinary frames (the oracle's default weighted tree, its gradient
    tree, explicit small trees) in ONE batch.  The ordinary frames come back exact from the global form too."""
    small = [c for c in M.families() if (c.family, c.name) in (("row trees", "rows"), ("cells", "1728"))]
    assert len(small) == 2
    srcs = [rgb(257, 200, 3), rgb(130, 67, 11), synth(300, 300, 12), small[0].image(65, 66), small[1].image(130, 67)]
    files = [oracle.encode(srcs[0], lossless=True, tree=big_tree(10, 4800, [5, 4, 7])),
             oracle.encode(srcs[1], lossless=True),
             oracle.encode(srcs[2], lossless=True, lossless_tree=1, lossless_predictor=5),
             oracle.encode(srcs[3], tree=small[0].nodes(65, 66), **small[0].encode_args()),
             oracle.encode(srcs[4], tree=small[1].nodes(130, 67), **small[1].encode_args())]
    for f in files[1:]:
        assert not plan_of([f])["mod_global"]
    for shape in ("default", "mod_lanes64"):
        P = assert_mod_plan(files, shape, LANES_WP, 256, 1)
        assert [f["tree_nodes"] > 9000 for f in P["frames"]] == [True, False, False, False, False]
    got = launch_shapes(gpu_decoder, files, together=True)
    assert set(got) == {"default", "mod_lanes64"}
    for shape, outs in got.items():
        for i, (g, s) in enumerate(zip(outs, srcs)):
            assert g.dtype == s.dtype and g.tobytes() == s.tobytes(), (shape, i, int((g != s).sum()))


# ---- wide codes: tiny frames whose alias tables, not their tree, leave LDS
def _wide_walk(w, h):
    return M.flatten(spread_tree(10, 128, 3, [5, 4, 7, 1]))


def _wide_weighted(w, h):
    return M.flatten(M.S(15, 0, spread_tree(10, 64, 6, [6, 5, 4, 7]), spread_tree(10, 64, 6, [7, 6, 1, 5])))


def _wide_static(w, h):
    """A leaf of its own for every (channel, row): properties 0 and 2 only, predictors 0 / 1 / 2 / 5."""
    rows = lambda c: M.buckets(2, list(range(h - 1)), [M.L((0, 1, 2, 5)[(c + y) % 4]) for y in range(h)])   # noqa: E731
    return M.flatten(M.buckets(0, [0, 1, 2], [rows(c) for c in range(4)]))


WIDE_TREES = {"walk": (_wide_walk, LANES_PLAIN, 256, 0), "weighted": (_wide_weighted, LANES_WP, 256, 1), "static": (_wide_static, LANES_PLAIN, 0, 0)}
# (63, 5) has 20 (channel, row) pairs: a row-static tree cannot fill 80 contexts there
WIDE = [((63, 5), "walk"), ((63, 5), "weighted"), ((65, 66), "walk"), ((65, 66), "weighted"), ((65, 66), "static")]


def wide_frame(oracle, size, kind):
    w, h = size
    src = noise(w, h, 4, 100 + w + h)
    return src, oracle.encode(src, lossless=True, tree=WIDE_TREES[kind][0](w, h), wide_codes=True)


@pytest.mark.parametrize("size,kind", WIDE, ids=["%dx%d %s" % (s[0], s[1], k) for s, k in WIDE])
def test_tiny_lossless_frame_with_wide_codes(gpu_decoder, oracle, size, kind):
    src, data = wide_frame(oracle, size, kind)
    _, lanes, rb, wp = WIDE_TREES[kind]
    f = plan_of([data])["frames"][0]
    clusters, log_alpha, _, prefix = f["mcode"]
    assert clusters >= 80 and log_alpha == 8 and not prefix and f["single"]
    assert 16 * f["tree_nodes"] < 16 * 1024   # the alias tables (2 KB per cluster) are what does not fit
    check_lossless(gpu_decoder, oracle, src, data, lanes, rb, wp)


@pytest.mark.parametrize("kind", list(WIDE_TREES))
def test_frame_of_six_pixels_in_a_launch_with_global_tables(gpu_decoder, oracle, kind):
    """2 x 3 RGBA has 24 samples and cannot fill 80 contexts itself: it shares its launch with the 65 x 66 frame of the same kind, whose
    tables take the launch to the global form (its own code is written with the knob as well: log_alpha 8, a few clusters)."""
    src, data = wide_frame(oracle, (2, 3), kind)
    big_src, big = wide_frame(oracle, (65, 66), kind)
    assert np.array_equal(oracle.decode(data).pixels, src)
    f = plan_of([data])
    assert not f["mod_global"] and f["frames"][0]["mcode"][1] == 8
    _, lanes, rb, wp = WIDE_TREES[kind]
    for shape in ("default", "mod_lanes64"):
        assert_mod_plan([data, big], shape, lanes, rb, wp)
    for shape, (g, gb) in launch_shapes(gpu_decoder, [data, big], together=True).items():
        assert g.tobytes() == src.tobytes() and gb.tobytes() == big_src.tobytes(), shape


# ================================================================ b. lf_ans_kernel<false> and alpha_ans_kernel<false>
# 264x264: four groups, edge groups 8 pixels wide, alpha in the pass groups; 256x256: one section, alpha in the global stream (decoded
# by lf_ans_kernel) and the 64-slot LF pre-pass of decoder.cc; 520x264: three group columns
LOSSY_SIZES = [(264, 264), (256, 256), (520, 264)]
# alpha tree (None: the writer's default, one gradient leaf), LF tree, lean_mod.  The writer appends the alpha tree twice and the LF
# tree three times: 2 * 4001 + 3 * 801 + 12 and 3 * 3201 + 14 nodes
LOSSY_TREES = {
    "per-sample": (lambda: big_tree(10, 2000, [5, 4, 7]), lambda: big_tree(9, 400, [5, 4, 7, 1]), 0),
    "property 2": (lambda: big_tree(2, 2000, [5, 1, 2, 0]), lambda: big_tree(2, 400, [5, 1, 2, 0]), 1),
    "big LF tree, default alpha": (lambda: None, lambda: big_tree(9, 1600, [5, 4, 7, 1]), 0),
}
LOSSY = [(s, k) for s in LOSSY_SIZES for k in LOSSY_TREES]


def options(dec, **opts):
    """Sets decoder options for one `with` block and puts the defaults back."""
    import contextlib
    defaults = dict(no_direct=0, lane_stride=0, band_first_row=0, band_rows=0)

    @contextlib.contextmanager
    def ctx():
        try:
            for k, v in opts.items():
                assert dec.set_option(k, v) or v == 0, k
            yield
        finally:
            for k in opts:
                dec.set_option(k, defaults[k])
    return ctx()


@pytest.fixture(scope="module")
def lossy(gpu_decoder, oracle):
    """Per size: the source, the file written with the default tree, the GPU's decode of it, the oracle's dump; per (size, trees) the file."""
    memo = {}

    def get(size, kind=None):
        w, h = size
        if size not in memo:
            img = synth(w, h, 40 + w)
            plain = oracle.encode(img, distance=1.0)
            assert not any(plan_of([plain])[k] for k in ("lf_global", "alpha_global", "hf_global"))
            memo[size] = (img, plain, batch(gpu_decoder, [plain])[0], oracle.decode(plain, want_dump=True))
        if kind is None:
            return memo[size]
        if (size, kind) not in memo:
            alpha_tree, lf_tree, _ = LOSSY_TREES[kind]
            memo[(size, kind)] = oracle.encode(memo[size][0], distance=1.0, alpha_tree=alpha_tree(), lf_tree=lf_tree())
        return memo[size] + (memo[(size, kind)],)
    return get


def assert_lossy_plan(files, lean, **opts):
    P = plan_of(files, **opts)
    lds_max = constants()["lds_max"]
    assert all(f["decoded"] and f["has_alpha"] for f in P["frames"])
    assert P["lf_global"] == 1 and P["alpha_global"] == 1 and P["hf_global"] == 0, opts
    assert P["lds_lf"] > lds_max and P["lds_alpha"] > lds_max and P["lean_mod"] == lean
    stride = opts.get("lane_stride", 0)
    assert (P["lane_stride"], P["alpha_stride"]) == ((stride, stride) if stride else (64, 64))
    direct = int(not opts.get("no_direct"))
    assert (P["direct_lf"], P["direct_alpha"]) == (direct, direct if not stride or stride == 64 else 0), opts
    return P


@pytest.mark.parametrize("size,kind", LOSSY, ids=["%dx%d %s" % (s[0], s[1], k) for s, k in LOSSY])
def test_lossy_frame_with_trees_too_big_for_lds(gpu_decoder, oracle, lossy, size, kind):
    img, plain, plain_px, plain_dump, data = lossy(size, kind)
    lean = LOSSY_TREES[kind][2]
    assert data != plain
    P = assert_lossy_plan([data], lean)
    f = P["frames"][0]
    assert f["single"] == int(size == (256, 256))
    if f["single"]:   # the pre-pass that finds a one-section frame's HfGlobal lays 64 slots out (decoder.cc) and makes the same choice
        assert layout(2, 64, f["tree_nodes"], *f["mcode"])[6] > constants()["lds_max"]
    # (with the stage taps on the pixel kernels run in another form, whose colour bytes differ by rounding: this decode is for the planes)
    batch(gpu_decoder, [data], taps=True)
    for c in range(3):
        assert np.array_equal(gpu_decoder.read_plane(0, "lf_quant", c), plain_dump.planes["lf_quant"][c]), c
    assert np.array_equal(gpu_decoder.read_plane(0, "alpha").astype(np.int32).ravel(), plain_dump.planes["alpha"].ravel())
    got = batch(gpu_decoder, [data])[0]
    assert np.array_equal(got[..., 3], img[..., 3])
    assert got.tobytes() == plain_px.tobytes()
    assert_lossy_plan([data], lean, no_direct=True)
    with options(gpu_decoder, no_direct=1):
        assert batch(gpu_decoder, [data])[0].tobytes() == plain_px.tobytes()
    assert_lossy_plan([data], lean, lane_stride=2)
    assert batch(gpu_decoder, [data], lane_stride=2)[0].tobytes() == plain_px.tobytes()
    # a plain frame between big ones: one launch, one form
    four = [data, plain, data, data]
    assert_lossy_plan(four, lean)
    assert all(f.tobytes() == plain_px.tobytes() for f in batch(gpu_decoder, four))
    assert_lossy_plan(four, lean, no_direct=True)
    with options(gpu_decoder, no_direct=1):
        assert all(f.tobytes() == plain_px.tobytes() for f in batch(gpu_decoder, four))


@pytest.mark.parametrize("size", [(264, 264), (520, 264)], ids=["264x264", "520x264"])
@pytest.mark.parametrize("stride", [2, 64])
def test_alpha_in_one_pass_with_global_tables(gpu_decoder, oracle, lossy, size, stride):
    """The default alpha leaf under a big LF tree: the groups stay eligible for the one-pass path (test_gpu_alpha_one_pass) while the
    launch's tables are global - the lanes' previous rows then lie straight behind the bit windows - and the redo launch decodes the
    groups a limit gives up, in the global form too."""
    img, plain, plain_px, _, data = lossy(size, "big LF tree, default alpha")
    assert_lossy_plan([data], 0, no_direct=True, lane_stride=stride)
    eligible = eligible_groups(*size)
    assert eligible > 0 and img[..., 3].max() > 200
    free, narrow, redo = one_pass_decode(gpu_decoder, [data], lane_stride=stride)
    assert (narrow, redo) == (eligible, 0)
    assert free[0].tobytes() == plain_px.tobytes()
    for limits in (dict(sample_limit=200), dict(narrow_limit=100, sample_limit=200), dict(narrow_limit=1)):
        outs, narrow, redo = one_pass_decode(gpu_decoder, [data], lane_stride=stride, **limits)
        print("%s stride %d %s: eligible %d, one pass %d, redo %d" % (size, stride, limits, eligible, narrow, redo))
        assert narrow + redo == eligible and redo > 0, limits
        assert outs[0].tobytes() == free[0].tobytes(), limits
    two_pass, narrow, redo = one_pass_decode(gpu_decoder, [data], lane_stride=stride, narrow_limit=0)
    assert (narrow, redo) == (0, 0) and two_pass[0].tobytes() == free[0].tobytes()
    # the per-sample alpha tree is not eligible: no group is counted, the bytes are the same
    other = lossy(size, "per-sample")[4]
    assert_lossy_plan([other], 0, no_direct=True, lane_stride=stride)
    outs, narrow, redo = one_pass_decode(gpu_decoder, [other], lane_stride=stride)
    assert (narrow, redo) == (0, 0) and outs[0].tobytes() == plain_px.tobytes()


@pytest.mark.parametrize("kind", ["per-sample", "big LF tree, default alpha"])
def test_band_of_a_frame_with_global_tables(gpu_decoder, oracle, kind):
    """264 x 520 (the 520 x 264 picture turned): three group rows; the middle one decoded as a band equals those rows of the whole."""
    img = np.ascontiguousarray(synth(520, 264, 40 + 520).transpose(1, 0, 2))
    assert img.shape == (520, 264, 4)
    alpha_tree, lf_tree, lean = LOSSY_TREES[kind]
    data = oracle.encode(img, distance=1.0, alpha_tree=alpha_tree(), lf_tree=lf_tree())
    plain = oracle.encode(img, distance=1.0)
    P = assert_lossy_plan([data], lean, band=(1, 1))
    assert P["frames"][0]["yg"] == 3 and [t for t in P["alpha"]] == [(0, 2, 1), (0, 3, 1)]
    whole = batch(gpu_decoder, [data])[0]
    assert np.array_equal(whole[..., 3], img[..., 3]) and whole.tobytes() == batch(gpu_decoder, [plain])[0].tobytes()
    with options(gpu_decoder, band_first_row=1, band_rows=1):
        import torch
        out = torch.zeros(256 * 264 * 4, dtype=torch.uint8, device="cuda")
        assert gpu_decoder.decode_batch([data], [out.data_ptr()], None, synchronize=True) == [0]
    band = out.cpu().numpy().reshape(256, 264, 4)
    assert band.tobytes() == whole[256:512].tobytes(), int((band != whole[256:512]).sum())
    assert_lossy_plan([data], lean, band=(1, 1), no_direct=True, lane_stride=2)
    outs, narrow, redo = one_pass_decode(gpu_decoder, [data], band=(1, 1))
    assert outs[0].tobytes() == band.tobytes()
    assert (narrow, redo) == ((1, 0) if alpha_tree() is None else (0, 0))   # the band's one group 256 wide


@pytest.mark.parametrize("size", [(264, 264), (256, 256)], ids=["264x264", "256x256"])
def test_reduced_size_decode_of_a_frame_with_global_tables(gpu_decoder, oracle, lossy, size):
    """downscale = 8 reads the LF image and, for the alpha behind them, the HF tokens: the LF and alpha launches in their global form."""
    img, plain, _, _, data = lossy(size, "per-sample")
    assert_lossy_plan([data], 0, downscale=8)
    got = DU.decode_reduced(gpu_decoder, data)
    assert np.array_equal(got[..., 3], DU.box_mean_int(img[..., 3]))
    assert got.tobytes() == DU.decode_reduced(gpu_decoder, plain).tobytes()


# ================================================================ c. hf_decode_kernel<false> with plain ANS codes
def _flat(w, h):
    img = np.full((h, w, 4), 120, np.uint8)
    img[..., 3] = 255
    return img


def _full_blocks(w, h):
    img = noise(w, h, 4, 1)
    img[..., 3] = 255
    return img


# 520x300 is six groups.  (name, pictures, encode options): every picture of a case goes into ONE launch
HF = [
    # a frame of one group and a flat frame (zero tokens: a handful of used contexts, tables that would fit) ride in the six-group
    # frame's launch: its 255 clusters of 2 KB take the launch to the global form
    ("mixed varblocks + one group + flat", [synth(520, 300, 3), synth(200, 120, 4), _flat(520, 300)], dict(strategy_mode=2)),
    ("two passes", [synth(520, 300, 5)], dict(strategy_mode=2, num_passes=2)),
    ("custom orders", [synth(520, 300, 6)], dict(strategy_mode=2, custom_orders=True)),
    ("lf contexts", [synth(520, 300, 7)], dict(strategy_mode=2, lf_contexts=True)),
    ("noise of full blocks", [_full_blocks(520, 300)], dict(distance=0.1, strategy_mode=1)),
]
# 0 / 64: one section per wavefront, HfGeneralLoop<false> entering HfScalarRun<false>; 2 and 8: HfBatchedLoop<false>
STRIDES = (0, 64, 2, 8)


@pytest.fixture(scope="module")
def hf_files(oracle):
    memo = {}

    def get(name):
        if name not in memo:
            _, pictures, enc = next(c for c in HF if c[0] == name)
            wide = [oracle.encode(p, wide_codes=True, **enc) for p in pictures]
            plain = [oracle.encode(p, **enc) for p in pictures]
            dumps = [oracle.decode(f, want_dump=True) for f in wide]
            # the knob changes the coding and nothing else
            for w, p, d in zip(wide, plain, dumps):
                assert w != p
                pd = oracle.decode(p, want_dump=True)
                same_planes(d, pd)
                assert np.array_equal(d.pixels, pd.pixels)
            memo[name] = (wide, plain, dumps)
        return memo[name]
    return get


@pytest.mark.parametrize("name", [c[0] for c in HF])
def test_hf_decoder_with_plain_ans_tables_in_global_memory(gpu_decoder, oracle, hf_files, name):
    wide, plain, dumps = hf_files(name)
    assert not plan_of(plain)["hf_global"]
    base = None
    for stride in STRIDES:
        P = plan_of(wide, lane_stride=stride)
        assert P["hf_global"] == 1 and P["lds_hf"] > constants()["lds_max"] and P["lane_stride"] == (stride or 64), stride
        assert not (P["lf_global"] or P["alpha_global"])
        f = P["frames"][0]
        assert f["ng"] == 6 and len(f["acodes"]) == f["num_passes"]
        for clusters, log_alpha, _, prefix in f["acodes"]:
            assert clusters >= 80 and log_alpha == 8 and not prefix   # plain ANS: not the general reader's prefix / LZ77 path
        outs = gpu_decode(gpu_decoder, wide, taps=True, lane_stride=stride)
        for i, (o, d) in enumerate(zip(outs, dumps)):
            check_report(compare_stages(gpu_decoder, i, d))   # qcoef bit-exact, every other integer plane too
            check_pixels(o, d.pixels)
        got = gpu_decode(gpu_decoder, wide, lane_stride=stride)
        want = gpu_decode(gpu_decoder, plain, lane_stride=stride)   # the pixel stages never see the entropy coding
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.tobytes() == w.tobytes(), (stride, i, int((g != w).sum()))
        if base is None:
            base = got
        for g, b in zip(got, base):
            assert g.tobytes() == b.tobytes(), stride


@pytest.mark.parametrize("size", [(264, 264), (256, 256)], ids=["264x264", "256x256"])
def test_every_launch_of_a_lossy_frame_with_global_tables(gpu_decoder, oracle, size):
    """Small trees with many leaves (129 on alpha, 65 on each LF channel), noise for alpha and the knob: the frame's Modular code keeps
    over a hundred clusters of 2 KB apart and its HF code 255, so the LF, alpha and HF launches all leave LDS because of alias tables."""
    w, h = size
    img = synth(w, h, 40 + w)
    img[..., 3] = noise(w, h, 1, 7)[..., 0]
    data = oracle.encode(img, distance=1.0, alpha_tree=_wide_walk(w, h), lf_tree=M.flatten(spread_tree(9, 64, 4, [5, 4, 7, 1])), wide_codes=True)
    plain = oracle.encode(img, distance=1.0)
    od, pd = oracle.decode(data, want_dump=True), oracle.decode(plain, want_dump=True)
    same_planes(od, pd, ("qcoef", "lf_quant", "strategy", "raw_quant", "alpha"))
    single = int(size == (256, 256))

    def assert_plan(files, **opts):
        P = plan_of(files, **opts)
        f = P["frames"][0]
        assert (P["lf_global"], P["alpha_global"], P["hf_global"], P["lean_mod"]) == (1, 1, 1 - single, 0), opts   # (one section: its HF code is found by the pre-pass, not planned)
        assert f["single"] == single and f["mcode"][0] >= 80 and f["mcode"][1] == 8 and 16 * f["tree_nodes"] < 16 * 1024
        assert single or (f["acodes"][0][0] >= 80 and f["acodes"][0][1] == 8 and not f["acodes"][0][3])
        assert P["lane_stride"] == (opts.get("lane_stride") or 64) and P["direct_lf"] == int(not opts.get("no_direct"))
    assert not any(plan_of([plain])[k] for k in ("lf_global", "alpha_global", "hf_global"))
    for files, opts in (([data], dict()), ([data], dict(no_direct=True)), ([data], dict(lane_stride=2)), ([data, plain, data], dict())):
        assert_plan(files, **opts)
    want = batch(gpu_decoder, [plain])[0]
    out = gpu_decode(gpu_decoder, [data], taps=True)[0]
    check_report(compare_stages(gpu_decoder, 0, od))
    check_pixels(out, od.pixels)
    got = batch(gpu_decoder, [data])[0]
    assert np.array_equal(got[..., 3], img[..., 3]) and got.tobytes() == want.tobytes()
    with options(gpu_decoder, no_direct=1):
        assert batch(gpu_decoder, [data])[0].tobytes() == want.tobytes()
    assert batch(gpu_decoder, [data], lane_stride=2)[0].tobytes() == want.tobytes()
    assert all(g.tobytes() == want.tobytes() for g in batch(gpu_decoder, [data, plain, data]))


def test_wide_code_that_still_fits_lds(gpu_decoder, oracle):
    """Two ramps use some thirty contexts: with the knob their code has log_alpha 8 - a width the writer never chose before - and stays
    in LDS (hf_decode_kernel<true>).  Same checks."""
    yy, xx = np.mgrid[0:264, 0:264]
    img = np.stack([xx * 255 // 263, yy * 255 // 263, np.full_like(xx, 128), np.full_like(xx, 255)], -1).astype(np.uint8)
    wide, plain = oracle.encode(img, wide_codes=True), oracle.encode(img)
    dw, dp = oracle.decode(wide, want_dump=True), oracle.decode(plain, want_dump=True)
    same_planes(dw, dp)
    for stride in (0, 2):
        P = plan_of([wide], lane_stride=stride)
        clusters, log_alpha, _, prefix = P["frames"][0]["acodes"][0]
        assert not P["hf_global"] and P["lds_hf"] <= constants()["lds_max"] and log_alpha == 8 and 8 < clusters < 80 and not prefix
        assert plan_of([plain])["frames"][0]["acodes"][0][1] < 8
        out = gpu_decode(gpu_decoder, [wide], taps=True, lane_stride=stride)[0]
        check_report(compare_stages(gpu_decoder, 0, dw))
        check_pixels(out, dw.pixels)
        assert gpu_decode(gpu_decoder, [wide], lane_stride=stride)[0].tobytes() == gpu_decode(gpu_decoder, [plain], lane_stride=stride)[0].tobytes()
