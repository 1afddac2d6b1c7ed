"""CPU tests of the entropy stage's arithmetic (no GPU): the LDS layouts the serial kernels carve by (csrc/lds_layout.h) and the launch
plan of a batch (csrc/entropy_plan.h), through two exports of the test library.  What a layout must look like - the order of its pieces,
their sizes and alignment - and which sections a call must decode are written out here on their own, not taken from the code under test."""
import ctypes as C
import itertools

import numpy as np
import pytest

from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth

_L = None


def _lib():
    global _L
    if _L is None:
        _L = api.selftest_lib()
        _L.jxlhip_selftest_lds_layout.restype = C.c_int32
        _L.jxlhip_selftest_lds_layout.argtypes = [C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        _L.jxlhip_selftest_entropy_plan.restype = C.c_size_t
        _L.jxlhip_selftest_entropy_plan.argtypes = [C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                                     C.c_size_t]
    return _L


_out = (C.c_int64 * 16)()


def layout(kind, *nums):
    arr = (C.c_int64 * max(1, len(nums)))(*nums)
    k = _lib().jxlhip_selftest_lds_layout(kind, arr, _out)
    assert k > 0
    return _out[:k]


def constants():
    names = ["lds_max", "ring_words", "hf_ring_words", "nzcol", "nnz_ctx", "wp_ints", "uni_rows", "uni_grid", "tree_node"]
    return dict(zip(names, layout(5)))


# ---------------------------------------------------------------- layouts
# a code's shape: (clusters, log_alpha, contexts, prefix)
SHAPES = [(cl, la, ctx, 0) for cl in range(1, 17) for la in (5, 6, 7, 8) for ctx in (1, 7, 9, 495 * 15)] + \
         [(cl, 15, ctx, 1) for cl in range(1, 17) for ctx in (1, 7, 9, 495 * 15)]
TREES = [1, 2, 3, 1023]


def check_pieces(starts, sizes, end, first, aligns):
    """The pieces lie in the given order without overlap, each at its alignment and no further from the piece before than that
    alignment asks; `end` is where the last one ends."""
    at = first
    for s, n, a in zip(starts, sizes, aligns):
        assert s % a == 0 and at <= s < at + a, (starts, sizes, first)
        at = s + n
    assert end == at, (starts, sizes, end)


def code_sizes(shape):
    cl, la, ctx, prefix = shape
    return [0 if prefix else 8 * (cl << la), 4 * cl, ctx]


def test_code_tables_layout():
    for shape in SHAPES:
        for off in (0, 1, 7, 8, 4100, 12345):
            alias, cfg, cmap, end, host = layout(0, off, *shape)
            check_pieces([alias, cfg, cmap], code_sizes(shape), end, off, [8, 1, 1])
            assert end - off <= host


def test_tree_and_code_layout():
    c = constants()
    assert c["tree_node"] == 16
    for shape in SHAPES:
        for nodes in TREES:
            for off in (0, 1, 15, 16, 128, 8192 + 3 * 1024 + 9):
                tree, alias, cfg, cmap, end, host = layout(1, off, nodes, *shape)
                check_pieces([tree, alias, cfg, cmap], [16 * nodes] + code_sizes(shape), end, off, [16, 8, 1, 1])
                assert end - off <= host


def test_lf_and_alpha_layout():
    c = constants()
    for shape in SHAPES:
        for nodes in TREES:
            for slots in (1, 4, 63, 64):
                win, tree, alias, cfg, cmap, end, host, lanes_only = layout(2, slots, nodes, *shape)
                check_pieces([win, tree, alias, cfg, cmap], [slots * c["ring_words"] * 4, 16 * nodes] + code_sizes(shape), end, 0, [16, 16, 8, 1, 1])
                assert end <= host and lanes_only == slots * c["ring_words"] * 4


def test_modular_layout():
    c = constants()
    for lanes, rb, wp, uniform in itertools.product((1, 8, 64), (0, 256), (0, 1), (0, 1)):
        if uniform and not (lanes == 1 and rb > 0):
            continue   # the uniform shape is the one-section-per-wavefront shape with row buffers
        sizes = [64 * c["ring_words"] * 4, (c["uni_rows"] if uniform else lanes) * rb * 4, lanes * c["wp_ints"] * (rb + 2) * 4 if wp else 0,
                 c["uni_grid"] if uniform else 0]
        for shape in SHAPES:
            for nodes in TREES:
                win, rows, wps, grid, tree, alias, cfg, cmap, end, host, lanes_only = layout(3, lanes, rb, wp, uniform, nodes, *shape)
                check_pieces([win, rows, wps, grid, tree, alias, cfg, cmap], sizes + [16 * nodes] + code_sizes(shape), end, 0, [16, 4, 4, 4, 16, 8, 1, 1])
                assert end <= host
                # the variant with its tables in global memory never takes the uniform shape
                assert lanes_only == 64 * c["ring_words"] * 4 + lanes * rb * 4 + (lanes * c["wp_ints"] * (rb + 2) * 4 if wp else 0)


def test_hf_layout():
    c = constants()
    ring = c["hf_ring_words"]
    for shape in SHAPES:
        for sections in range(1, 513):
            if sections % 4 not in (0, 1):
                continue   # every multiple of four up to 512, and the counts just above one (rounded up by the layout)
            ringo, descq, nzcol, alias, cfg, cmap, nnz, end, host, lanes_only, slots = layout(4, sections, *shape)
            assert slots == (sections + 3) // 4 * 4
            check_pieces([ringo, descq, nzcol, alias, cfg, cmap, nnz], [slots * ring * 4, slots * 2 * (ring // 4) * 4, slots * c["nzcol"]] + code_sizes(shape) + [c["nnz_ctx"]],
                         end, 0, [16, 4, 1, 8, 1, 1, 1])
            assert end <= host and lanes_only == alias and lanes_only == slots * (ring * 4 + ring * 2 + c["nzcol"])


# ---------------------------------------------------------------- plans
HEAD = ["n", "n_extra", "global_direct", "lean_mod", "lane_stride", "hf_waves", "alpha_stride", "per_alpha_wg", "lf_per_wave", "mod_lanes", "mod_rb",
        "mod_wp_lds", "direct_lf", "direct_alpha", "direct_mod", "lds_lf", "lf_global", "lds_hf", "hf_global", "lds_hf_lanes", "lds_alpha", "alpha_global",
        "lds_mod", "mod_global", "max_mod_groups", "max_mod_coded"]
FRAME = ["status", "decoded", "encoding", "single", "xg", "yg", "ng", "xlf", "ylf", "nlf", "num_passes", "has_alpha", "ysize", "tree_nodes", "tree_row_static",
         "tree_uses_wp", "dec_gy0", "dec_gy1", "band_y0", "band_y1", "lf0", "lf1", "hf0", "hf1", "alpha0", "alpha1", "hf", "first_extra", "hf_per_wg",
         "hf_table_bytes"]
TABLES = ["lf_finish", "lf_ans", "pass", "alpha", "mod"]


def plan_of(files, band=(0, 0), downscale=1, lane_stride=0, no_direct=False, mod_lanes64=False):
    n = len(files)
    data = (C.c_char_p * n)(*files)
    sizes = (C.c_size_t * n)(*[len(f) for f in files])
    opts = (C.c_int32 * 6)(band[0], band[1], downscale, lane_stride, int(no_direct), int(mod_lanes64))
    cap = 1 << 20
    while True:
        buf = np.zeros(cap, np.int64)
        k = _lib().jxlhip_selftest_entropy_plan(n, data, sizes, opts, buf.ctypes.data_as(C.POINTER(C.c_int64)), cap)
        if k:
            break
        cap *= 4
        assert cap <= 1 << 26
    v = buf[:k].tolist()
    pos = [0]

    def take(m):
        pos[0] += m
        return v[pos[0] - m:pos[0]]
    P = dict(zip(HEAD, take(len(HEAD))))
    P["frames"] = []
    for _ in range(n):
        f = dict(zip(FRAME, take(len(FRAME))))
        f["mcode"] = tuple(take(4))
        f["acodes"] = [tuple(take(4)) for _ in range(take(1)[0])]
        f["sec_size"] = take(take(1)[0])
        P["frames"].append(f)
    for name in TABLES:
        m = take(1)[0]
        flat = take(3 * m)
        P[name] = [tuple(flat[3 * j:3 * j + 3]) for j in range(m)]
    P["hf_orders"] = {}
    for _ in range(take(1)[0]):
        image, p, m = take(3)
        assert (image, p) not in P["hf_orders"]
        P["hf_orders"][(image, p)] = take(m)
    assert pos[0] == k
    return P


def covered_once(tasks, image, want, lanes):
    """The tasks of `image` hold every section of `want` exactly once and nothing else; none is wider than a workgroup."""
    got = []
    for im, first, count in tasks:
        if im == image:
            assert 1 <= count <= lanes, (count, lanes)
            got += range(first, first + count)
    assert sorted(got) == sorted(want), (image, got, list(want))


def check_plan(P, band=(0, 0), downscale=1):
    c = constants()
    n = P["n"]
    frames = P["frames"]
    assert 64 % P["lane_stride"] == 0 and 64 % P["alpha_stride"] == 0 and P["per_alpha_wg"] == 64 // P["alpha_stride"]
    assert 1 <= P["lf_per_wave"] <= 64 and P["mod_lanes"] in (1, 8, 64) and 1 <= P["hf_waves"] <= 8
    hf_lanes = P["hf_waves"] * (64 // P["lane_stride"])
    assert hf_lanes <= 512   # hf_decode_kernel's launch bound
    # the scalar-unit row loops are for wavefronts of one section
    assert not P["direct_lf"] or (P["global_direct"] and P["lf_per_wave"] == 1)
    assert not P["direct_alpha"] or (P["global_direct"] and P["per_alpha_wg"] == 1)
    assert not P["direct_mod"] or (P["global_direct"] and P["mod_lanes"] == 1)
    # a launch asks for no more LDS than the limit, or keeps its tables in global memory - and only then: the plan has no other reason
    # to leave LDS.  The `streams` below reach that form in the HF launch alone (LZ77); `global_streams` take every launch there, and
    # check_global_launches states what those launches are handed
    for k in ("lf", "hf", "alpha", "mod"):
        assert P[k + "_global"] == int(P["lds_" + k] > c["lds_max"]), k
    # image records: the batch's frames, then the later passes of the progressive ones
    rec_of = {}
    extra = 0
    for i, f in enumerate(frames):
        rec_of[i] = (i, 0)
        if f["decoded"] and f["encoding"] == 0:
            assert f["first_extra"] == n + extra
            for p in range(1, f["num_passes"]):
                rec_of[f["first_extra"] + p - 1] = (i, p)
            extra += f["num_passes"] - 1
    assert extra == P["n_extra"]
    # no task names a frame that is not decoded, or a record that does not exist
    for name in TABLES:
        for im, first, count in P[name]:
            assert im in rec_of and frames[rec_of[im][0]]["decoded"], (name, im)
            assert name == "pass" or im < n
    for (i, p) in P["hf_orders"]:
        assert frames[i]["decoded"]
    ds = downscale == 8
    for i, f in enumerate(frames):
        assert f["decoded"] == (f["status"] == 0)
        if not f["decoded"]:
            for name in TABLES:
                covered_once(P[name], i, [], 1)
            continue
        if f["encoding"] == 1:
            for name in ("lf_finish", "lf_ans", "pass", "alpha"):
                covered_once(P[name], i, [], 1)
            if f["single"]:
                assert [t for t in P["mod"] if t[0] == i] == [(i, 0, 1)]   # one lane walks the one bit stream
            else:
                covered_once(P["mod"], i, range(1 + f["nlf"] + f["ng"]), P["mod_lanes"])
            if not P["mod_global"]:
                uniform = int(P["mod_lanes"] == 1 and P["mod_rb"] > 0)
                end = layout(3, P["mod_lanes"], P["mod_rb"], P["mod_wp_lds"], uniform, f["tree_nodes"], *f["mcode"])[8]
                assert end <= P["lds_mod"]
            assert P["max_mod_groups"] >= 1 + f["nlf"] + f["ng"]
            # per-sample trees need the row buffers, the weighted predictor its state beside them
            if not f["tree_row_static"]:
                assert P["mod_rb"] == 256
            if f["tree_uses_wp"]:
                assert P["mod_wp_lds"] == 1 and P["mod_lanes"] <= 8
            continue
        covered_once(P["mod"], i, [], 1)
        # the band's group rows, one more each side for the loop filters' halo, and the LF groups those rows touch (8 group rows each)
        b0, b1 = 0, f["yg"]
        if band[1] > 0:
            b0 = min(band[0], f["yg"])
            b1 = min(b0 + band[1], f["yg"])
        g0, g1 = max(0, b0 - 1), min(f["yg"], b1 + 1)
        assert (f["dec_gy0"], f["dec_gy1"]) == (g0, g1)
        assert (f["band_y0"], f["band_y1"]) == (min(b0 * 256, f["ysize"]), min(b1 * 256, f["ysize"]))
        lf = [y * f["xlf"] + x for y in range(g0 // 8, (g1 + 7) // 8) for x in range(f["xlf"])]
        assert lf and max(lf) < f["nlf"] and (f["lf0"], f["lf1"]) == (lf[0], lf[-1] + 1)
        covered_once(P["lf_finish"], i, lf, 1)
        covered_once(P["lf_ans"], i, lf, P["lf_per_wave"])
        if not P["lf_global"]:
            assert layout(2, P["lf_per_wave"], f["tree_nodes"], *f["mcode"])[5] <= P["lds_lf"]
        # HF groups of the decoded rows, for every pass (reduced size: only to find the alpha stream behind them)
        hf = list(range(g0 * f["xg"], g1 * f["xg"]))
        assert (f["hf0"], f["hf1"]) == (hf[0], hf[-1] + 1) and f["hf"] == int(not ds or f["has_alpha"])
        assert len(f["acodes"]) == f["num_passes"]
        for p in range(f["num_passes"]):
            rec = i if p == 0 else f["first_extra"] + p - 1
            if not f["hf"]:
                covered_once(P["pass"], rec, [], 1)
                assert (i, p) not in P["hf_orders"]
                continue
            assert f["hf_per_wg"] <= hf_lanes
            covered_once(P["pass"], rec, range(len(hf)), f["hf_per_wg"])   # pass tasks index slots of the order
            order = P["hf_orders"][(i, p)]
            assert sorted(order) == hf
            if not f["single"]:   # largest section first, equal sizes in group order
                sec0 = 2 + f["nlf"] + p * f["ng"]
                assert order == sorted(hf, key=lambda g: -f["sec_size"][sec0 + g])
            # (the export plans without the LF pre-pass that locates a one-group frame's HfGlobal, as the plan allows: such a frame's HF
            # code is unread here, its tables are 0 bytes and this check only covers its lanes; the multi-group streams carry real tables)
            for im, first, count in P["pass"]:
                if im != rec:
                    continue
                lay = layout(4, count, *f["acodes"][p])
                if not P["hf_global"]:
                    assert lay[7] <= P["lds_hf"]
                assert lay[9] <= P["lds_hf_lanes"]
        # alpha: the band's own rows
        alpha = list(range(b0 * f["xg"], b1 * f["xg"])) if f["has_alpha"] else []
        covered_once(P["alpha"], i, alpha, P["per_alpha_wg"])
        if f["has_alpha"]:
            assert (f["alpha0"], f["alpha1"]) == (alpha[0], alpha[-1] + 1)
            if not P["alpha_global"]:
                assert layout(2, P["per_alpha_wg"], f["tree_nodes"], *f["mcode"])[5] <= P["lds_alpha"]
        # the lean kernels have no per-sample path
        if P["lean_mod"]:
            assert f["tree_row_static"] and not f["tree_uses_wp"] and not f["mcode"][3]


@pytest.fixture(scope="module")
def streams(oracle):
    def img(w, h, seed, nch=4):
        return np.ascontiguousarray(synth(w, h, seed)[..., :nch])
    S = {}
    S["8x8 rgb"] = oracle.encode(img(8, 8, 1, 3))
    S["8x8 rgba"] = oracle.encode(img(8, 8, 2))
    S["200x150 rgb"] = oracle.encode(img(200, 150, 3, 3))
    S["200x150 rgba"] = oracle.encode(img(200, 150, 4))
    S["257x257 rgba"] = oracle.encode(img(257, 257, 5))
    S["2049x8 rgb"] = oracle.encode(img(2049, 8, 6, 3))
    S["513x300 2 passes"] = oracle.encode(img(513, 300, 7), num_passes=2)
    S["513x300 3 passes"] = oracle.encode(img(513, 300, 8, 3), num_passes=3)
    for w, h in ((64, 64), (300, 300)):
        S["%dx%d lossless gradient" % (w, h)] = oracle.encode(img(w, h, 9), lossless=True, lossless_tree=1, lossless_predictor=5)
        S["%dx%d lossless weighted" % (w, h)] = oracle.encode(img(w, h, 10, 3), lossless=True)
    S["200x150 prefix"] = oracle.encode(img(200, 150, 11), prefix_codes=True)
    S["300x280 lz77"] = oracle.encode(img(300, 280, 12), lz77=True)
    S["300x280 lossless prefix+lz77"] = oracle.encode(img(300, 280, 13, 3), lossless=True, prefix_codes=True, lz77=True)
    # three group rows, for the band options
    S["64x600 rgba"] = oracle.encode(img(64, 600, 14))
    S["300x600 2 passes"] = oracle.encode(img(300, 600, 15), num_passes=2)
    return S


def test_streams_reach_the_shapes_they_are_meant_to(streams):
    P = plan_of(list(streams.values()))
    by = dict(zip(streams, P["frames"]))
    assert all(f["decoded"] for f in P["frames"])
    assert by["8x8 rgb"]["single"] and by["200x150 rgba"]["single"] and by["200x150 rgba"]["has_alpha"] and not by["200x150 rgb"]["has_alpha"]
    assert by["257x257 rgba"]["ng"] == 4 and (by["2049x8 rgb"]["nlf"], by["2049x8 rgb"]["ng"]) == (2, 9)
    assert by["513x300 2 passes"]["num_passes"] == 2 and by["513x300 3 passes"]["num_passes"] == 3
    for size in ("64x64", "300x300"):
        g, w = by[size + " lossless gradient"], by[size + " lossless weighted"]
        assert g["encoding"] == 1 and not g["tree_row_static"] and not g["tree_uses_wp"] and w["tree_uses_wp"]
    assert by["64x64 lossless gradient"]["single"] and not by["300x300 lossless gradient"]["single"]
    assert by["200x150 prefix"]["acodes"][0][3] == 1 and by["300x280 lz77"]["acodes"][0][3] == 0
    assert by["64x600 rgba"]["yg"] == 3 and by["300x600 2 passes"]["yg"] == 3


VARIANTS = [dict(), dict(lane_stride=1), dict(lane_stride=2), dict(lane_stride=64), dict(no_direct=True), dict(mod_lanes64=True), dict(downscale=8)]


@pytest.mark.parametrize("opts", VARIANTS, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()) or "defaults")
def test_plan_of_single_images_and_of_a_mixed_batch(streams, opts):
    batches = [[s] for s in streams.values()] + [list(streams.values())]
    for files in batches:
        P = plan_of(files, **opts)
        assert all(f["decoded"] for f in P["frames"])
        check_plan(P, downscale=opts.get("downscale", 1))
        if "lane_stride" in opts:
            assert P["lane_stride"] == opts["lane_stride"] and P["alpha_stride"] == opts["lane_stride"]
        if opts.get("no_direct"):
            assert not P["global_direct"] and not (P["direct_lf"] or P["direct_alpha"] or P["direct_mod"])
        if opts.get("mod_lanes64"):
            assert P["mod_lanes"] != 1
    # one frame, default options: one section per wavefront everywhere, rows on the scalar unit
    P = plan_of([streams["257x257 rgba"]])
    assert (P["lane_stride"], P["alpha_stride"], P["lf_per_wave"], P["global_direct"]) == (64, 64, 1, 1)
    P = plan_of([streams["300x300 lossless weighted"]])
    assert (P["mod_lanes"], P["mod_rb"], P["mod_wp_lds"], P["direct_mod"]) == (1, 256, 1, 1)
    # an LZ77 code keeps its 96 clusters apart: 200 KB of HF tables, which stay in global memory
    P = plan_of([streams["300x280 lz77"]])
    assert P["lds_hf"] > constants()["lds_max"] and P["hf_global"] and not (P["lf_global"] or P["alpha_global"])


@pytest.mark.parametrize("opts", VARIANTS[:6], ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()) or "defaults")
def test_plan_of_a_batch_of_thousands_of_sections(streams, opts):
    names = ["257x257 rgba", "2049x8 rgb", "513x300 2 passes", "513x300 3 passes", "300x300 lossless gradient", "300x300 lossless weighted", "300x600 2 passes",
             "300x280 lz77"]
    groups = 4 + 9 + 12 + 18 + 12 + 4
    files = [streams[k] for k in names] * (8192 // groups + 1)
    P = plan_of(files, **opts)
    assert sum((f["hf1"] - f["hf0"]) * f["num_passes"] for f in P["frames"] if f["encoding"] == 0) >= 8192
    check_plan(P)
    assert not P["global_direct"]
    if "lane_stride" not in opts:
        assert P["lane_stride"] == 2   # (the measured shape of large batches)
    assert P["mod_lanes"] == 8 and P["lf_per_wave"] > 1


@pytest.mark.parametrize("opts", VARIANTS[:5], ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()) or "defaults")
def test_plan_of_a_band(streams, opts):
    files = [streams["64x600 rgba"], streams["300x600 2 passes"]]
    for band in ((1, 1), (0, 1), (2, 1), (0, 3), (1, 5)):
        for batch in ([files[0]], [files[1]], files):
            P = plan_of(batch, band=band, **opts)
            check_plan(P, band=band)
    P = plan_of(files, band=(1, 1), **opts)
    f = P["frames"][0]
    assert (f["dec_gy0"], f["dec_gy1"], f["band_y0"], f["band_y1"]) == (0, 3, 256, 512)
    assert [t for t in P["alpha"] if t[0] == 0] == [(0, 1, 1)]   # (64 pixels wide: one group per row)


def test_frames_that_failed_to_parse_contribute_nothing(streams):
    good = streams["257x257 rgba"]
    files = [good, good[:40], b"\xff\x0a" + bytes(30), streams["300x300 lossless gradient"], good[:len(good) // 8]]
    P = plan_of(files)
    assert [f["decoded"] for f in P["frames"]] == [1, 0, 0, 1, 0]
    check_plan(P)
    assert {t[0] for name in TABLES for t in P[name]} == {0, 3}


# ---------------------------------------------------------------- launches whose tables stay in global memory
def big_tree(prop, n, preds):
    """n thresholds around zero on one property, the leaves' predictors cycling through `preds`: 2 n + 1 nodes of 16 bytes."""
    import ma_tree_util as M
    leaf = M.Leaves(preds)
    return M.flatten(M.buckets(prop, list(range(-(n // 2), n - n // 2)), [leaf() for _ in range(n + 1)]))


@pytest.fixture(scope="module")
def global_streams(oracle):
    """Files one of whose launches cannot hold its tables in LDS: trees of 4 901 .. 10 417 nodes, or codes written with log_alpha 8 and
    up to 255 clusters (oracle.encode(wide_codes=True): 2 KB of alias table per cluster).  tests/test_gpu_global_tables.py decodes them."""
    def img(w, h, seed, nch=4):
        return np.ascontiguousarray(synth(w, h, seed)[..., :nch])
    S = {}
    S["160x130 lossless, tree 4901"] = oracle.encode(img(160, 130, 1, 3), lossless=True, tree=big_tree(10, 2450, [5, 4, 7]))
    S["257x200 lossless, tree 9601 weighted"] = oracle.encode(img(257, 200, 5, 3), lossless=True, tree=big_tree(15, 4800, [6, 5, 4, 7]))
    S["257x200 lossless, tree 9601 row-static"] = oracle.encode(img(257, 200, 4, 3), lossless=True, tree=big_tree(2, 4800, [0, 1, 2, 5]))
    noise = np.random.default_rng(131).integers(0, 256, (66, 65, 4), dtype=np.uint8)
    S["65x66 lossless, wide code"] = oracle.encode(noise, lossless=True, tree=big_tree(10, 128, [5, 4, 7, 1]), wide_codes=True)
    S["264x264 rgba, alpha + LF trees"] = oracle.encode(img(264, 264, 40 + 264), alpha_tree=big_tree(10, 2000, [5, 4, 7]), lf_tree=big_tree(9, 400, [5, 4, 7, 1]))
    S["256x256 rgba, row-static trees"] = oracle.encode(img(256, 256, 40 + 256), alpha_tree=big_tree(2, 2000, [5, 1, 2, 0]), lf_tree=big_tree(2, 400, [5, 1, 2, 0]))
    S["520x264 rgba, LF tree"] = oracle.encode(img(520, 264, 40 + 520), lf_tree=big_tree(9, 1600, [5, 4, 7, 1]))
    S["520x300 rgba, wide code"] = oracle.encode(img(520, 300, 3), strategy_mode=2, wide_codes=True)
    S["520x300 rgba, wide code, 2 passes"] = oracle.encode(img(520, 300, 5), strategy_mode=2, num_passes=2, wide_codes=True)
    return S


def check_global_launches(P, want):
    """The launches named in `want`, and no others, keep their tables in global memory.  Such a launch is handed the lanes' bytes alone
    (the Launch* wrappers of entropy_kernels.hip ask the layouts for them): what the layouts report for the launch's shape must be what
    the lanes need by the arithmetic written out here, for every frame of the launch, and within the limit."""
    c = constants()
    ring = c["ring_words"] * 4
    assert {k for k in ("lf", "hf", "alpha", "mod") if P[k + "_global"]} == set(want)
    for f in P["frames"]:
        if not f["decoded"]:
            continue
        if f["encoding"] == 1 and P["mod_global"]:
            lanes, rb, wp = P["mod_lanes"], P["mod_rb"], P["mod_wp_lds"]
            handed = layout(3, lanes, rb, wp, 0, f["tree_nodes"], *f["mcode"])[10]   # (never the uniform shape)
            assert handed == 64 * ring + lanes * rb * 4 + (lanes * c["wp_ints"] * (rb + 2) * 4 if wp else 0) and handed <= c["lds_max"]
        if f["encoding"] == 0 and P["lf_global"]:
            assert layout(2, P["lf_per_wave"], f["tree_nodes"], *f["mcode"])[7] == P["lf_per_wave"] * ring <= c["lds_max"]
        if f["encoding"] == 0 and P["alpha_global"] and f["has_alpha"]:
            slots = P["per_alpha_wg"]
            rows, end = layout(6, slots, f["tree_nodes"], *f["mcode"])[4:6]   # the one-pass rows straight behind the bit windows
            assert (rows, end) == (slots * ring, slots * ring + slots * 256) and end <= c["lds_max"]
            assert layout(2, slots, f["tree_nodes"], *f["mcode"])[7] == slots * ring   # launches without the one-pass rows
    if P["hf_global"]:
        lanes = [layout(4, count, 1, 8, 1, 0)[9] for _, _, count in P["pass"]]   # (the lanes' bytes do not depend on the code)
        assert P["lds_hf_lanes"] == max(lanes) <= c["lds_max"]
        assert all(b == (count + 3) // 4 * 4 * (c["hf_ring_words"] * 4 + c["hf_ring_words"] * 2 + c["nzcol"]) for b, (_, _, count) in zip(lanes, P["pass"]))


GLOBAL_WANT = {"160x130 lossless, tree 4901": ["mod"], "257x200 lossless, tree 9601 weighted": ["mod"], "257x200 lossless, tree 9601 row-static": ["mod"],
               "65x66 lossless, wide code": ["mod"], "264x264 rgba, alpha + LF trees": ["lf", "alpha"], "256x256 rgba, row-static trees": ["lf", "alpha"],
               "520x264 rgba, LF tree": ["lf", "alpha"], "520x300 rgba, wide code": ["hf"], "520x300 rgba, wide code, 2 passes": ["hf"]}


@pytest.mark.parametrize("opts", VARIANTS, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()) or "defaults")
def test_plan_of_streams_whose_tables_do_not_fit_lds(streams, global_streams, opts):
    assert set(GLOBAL_WANT) == set(global_streams)
    ds = opts.get("downscale", 1)
    for name, data in global_streams.items():
        P = plan_of([data], **opts)
        assert all(f["decoded"] for f in P["frames"]), name
        check_plan(P, downscale=ds)
        # (a reduced-size decode of an opaque frame launches no HF decoder: nothing to keep anywhere)
        want = [k for k in GLOBAL_WANT[name] if not (k == "hf" and ds == 8 and not P["frames"][0]["hf"])]
        check_global_launches(P, want)
    by = {k: plan_of([v])["frames"][0] for k, v in global_streams.items()}
    assert by["160x130 lossless, tree 4901"]["tree_nodes"] == 4901 and by["160x130 lossless, tree 4901"]["single"]
    assert by["257x200 lossless, tree 9601 weighted"]["tree_uses_wp"] and by["257x200 lossless, tree 9601 row-static"]["tree_row_static"]
    assert by["65x66 lossless, wide code"]["mcode"][:2] == (129, 8) and by["65x66 lossless, wide code"]["tree_nodes"] == 257
    assert by["264x264 rgba, alpha + LF trees"]["tree_nodes"] == 2 * 4001 + 3 * 801 + 12 and by["256x256 rgba, row-static trees"]["single"]
    assert by["520x300 rgba, wide code"]["acodes"] == [(255, 8, 7425, 0)] and by["520x300 rgba, wide code, 2 passes"]["acodes"] == [(255, 8, 7425, 0)] * 2
    # one such frame takes the whole launch with it: every ordinary stream of this file in one batch with all of them
    files = list(streams.values()) + list(global_streams.values())
    P = plan_of(files, **opts)
    check_plan(P, downscale=ds)
    check_global_launches(P, ["lf", "hf", "alpha", "mod"])
    # ... and the ordinary streams with one of them at a time
    for name in ("160x130 lossless, tree 4901", "520x264 rgba, LF tree", "520x300 rgba, wide code"):
        P = plan_of(list(streams.values()) + [global_streams[name]], **opts)
        check_plan(P, downscale=ds)
        check_global_launches(P, sorted(set(GLOBAL_WANT[name]) | {"hf"}))   # (hf: the LZ77 stream of `streams`)
