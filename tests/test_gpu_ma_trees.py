"""GPU tests of the MA-tree decoders with explicit trees (ma_tree_util: every property, leaf form and grid shape): the two-phase path
of constant and row-static channels, ModularChannelUniform (grid in lanes, grid in LDS, tree-walk fallback), the per-lane walk of
ModularChannel in launches with many sections per wavefront, and the per-sample walk inside the LF and alpha kernels of lossy frames.
The ground truth of a lossless frame is its source; every launch shape must reproduce it bit for bit, and agree with the oracle."""
import numpy as np
import pytest

import ma_tree_util as M
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth

pytestmark = pytest.mark.gpu

CASES = M.families()
PAIRS = [(c, s) for c in CASES for s in c.sizes]


def batch(dec, files, taps=False, lane_stride=0):
    """One decode_batch; returns the images as arrays of the sample type peek reports."""
    import torch
    dec.set_option("debug_taps", 1 if taps else 0)
    dec.set_option("lane_stride", lane_stride)
    infos = [api.peek(f) for f in files]
    outs = [torch.zeros(i.width * i.height * i.num_channels * i.bytes_per_sample, dtype=torch.uint8, device="cuda") for i in infos]
    torch.cuda.synchronize()
    st = dec.decode_batch(files, [o.data_ptr() for o in outs])
    assert all(s == 0 for s in st), st
    return [o.cpu().numpy().view({1: np.uint8, 2: np.uint16, 4: np.float32}[i.bytes_per_sample]).reshape(i.height, i.width, i.num_channels)
            for o, i in zip(outs, infos)]


def launch_shapes(dec, files, together=False):
    """The same files through every launch shape: one section per wavefront (the default of a small launch), the per-lane walk with
    64 sections per wavefront (8 with the weighted predictor), and that without the per-residue tables."""
    run = (lambda: batch(dec, files)) if together else (lambda: [batch(dec, [f])[0] for f in files])
    out = {"default": run()}
    try:
        assert dec.set_option("mod_lanes64", 1)
        out["mod_lanes64"] = run()
        if not together:
            assert dec.set_option("no_direct", 1)
            out["mod_lanes64 + no_direct"] = run()
    finally:
        dec.set_option("no_direct", 0)
        dec.set_option("mod_lanes64", 0)
    return out


def encoded(oracle, case, w, h):
    src = case.image(w, h)
    return src, oracle.encode(src, tree=case.nodes(w, h), **case.encode_args())


@pytest.mark.parametrize("case,size", PAIRS, ids=["%s %dx%d" % (c.id, s[0], s[1]) for c, s in PAIRS])
def test_tree_family_is_bit_exact_in_every_launch_shape(gpu_decoder, oracle, case, size):
    w, h = size
    src, data = encoded(oracle, case, w, h)
    ref = oracle.decode(data).pixels
    assert np.array_equal(ref, src)
    one = api.load_image(data).pixels                      # LoadImage
    assert one.dtype == src.dtype and one.shape == src.shape
    assert one.tobytes() == src.tobytes(), "LoadImage: %d samples differ" % int((one != src).sum())
    for name, (got,) in launch_shapes(gpu_decoder, [data]).items():
        assert got.dtype == src.dtype and got.shape == src.shape, name
        bad = np.argwhere(got != src)
        assert got.tobytes() == src.tobytes(), "%s: %d samples differ, the first at (y, x, c) = %s" % (name, len(bad), tuple(bad[0]) if len(bad) else ())
        assert got.tobytes() == one.tobytes(), name


def test_six_families_in_one_batch(gpu_decoder, oracle):
    """Six frames of different sizes whose trees come from six families, in ONE launch (tables per image), with one section per
    wavefront and with 64."""
    pick = [("one property", "p12", (63, 5)), ("layout16", "4 props, 16", (65, 66)), ("cells", "1728", (130, 67)),
            ("static nodes", "squeezed", (257, 70)), ("leaf forms", "per-sample", (70, 257)), ("random", "weighted 3", (2, 3))]
    srcs, files = [], []
    for family, name, (w, h) in pick:
        case = next(c for c in CASES if c.family == family and c.name == name)
        src, data = encoded(oracle, case, w, h)
        srcs.append(src)
        files.append(data)
    for shape, got in launch_shapes(gpu_decoder, files, together=True).items():
        for (family, name, _), g, s in zip(pick, got, srcs):
            assert g.dtype == s.dtype and np.array_equal(g, s), (shape, family, name)


# ---------------------------------------------------------------- lossy frames: trees on the alpha channel and on the LF image
def _alpha_of_multiples(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return (96 * ((xx // 5 + yy // 3) % 3)).astype(np.uint8)


def _one(p, preds):
    return M.flatten(M.buckets(p, [-2, 0, 6], [M.L(q) for q in preds]))


def lossy_combos(w, h):
    """(name, alpha tree, LF tree, alpha of multiples of 96)"""
    w8, h8 = -(-w // 8), -(-h // 8)
    forms = M.Leaves([(4, 0, 2), (7, 0, 3), (8, 96, 4), (9, 0, 96), (5, 1, 1), (0, -1, 1), (1, -96, 96), (2, 0, 1)])
    return [("a p10, lf p9", _one(10, (4, 7, 8, 9)), _one(9, (1, 12, 13, 3)), False),
            ("a p12, lf p12", _one(12, (10, 11, 2, 5)), _one(12, (0, 4, 5, 7)), False),
            ("a p14, lf p13", _one(14, (13, 3, 1, 12)), _one(13, (8, 9, 10, 11)), False),
            ("a random, lf all 6 + p15", M.flatten(M.random_tree(301, False, w, h)), M.flatten(M.nest([(15, [-20, -3, 0, 2, 19])], M.Leaves([6]))), False),
            ("a leaf forms, lf random", M.flatten(M.nest([(10, [-96, 0, 95]), (3, [0, 64])], forms)), M.flatten(M.random_tree(302, True, w8, h8)), True),
            ("a random weighted, lf random", M.flatten(M.random_tree(303, True, w, h)), M.flatten(M.random_tree(304, False, w8, h8)), False)]


LOSSY = [(size, k) for size in ((130, 67), (257, 70)) for k in range(6)]


@pytest.fixture(scope="module")
def lossy_plain(gpu_decoder, oracle):
    """Per (size, alpha kind): the source, the file written with the default tree, the GPU's decode of it, the oracle's dump."""
    memo = {}

    def get(w, h, multiples):
        if (w, h, multiples) not in memo:
            img = synth(w, h, 40 + w)
            if multiples:
                img[..., 3] = _alpha_of_multiples(w, h)
            plain = oracle.encode(img, distance=1.0)
            memo[(w, h, multiples)] = (img, plain, batch(gpu_decoder, [plain])[0], oracle.decode(plain, want_dump=True))
        return memo[(w, h, multiples)]
    return get


@pytest.mark.parametrize("size,k", LOSSY, ids=["%dx%d %s" % (s[0], s[1], lossy_combos(*s)[k][0]) for s, k in LOSSY])
def test_lossy_frame_with_alpha_and_lf_trees(gpu_decoder, oracle, lossy_plain, size, k):
    """A tree changes the coding of a lossy frame, not its content: alpha is the source's, the quantised LF is the oracle's, and
    the decoded bytes are those of the GPU's own decode of the same picture written with the default tree."""
    from test_entropy_plan import plan_of
    w, h = size
    name, alpha_tree, lf_tree, multiples = lossy_combos(w, h)[k]
    img, plain, plain_px, plain_dump = lossy_plain(w, h, multiples)
    data = oracle.encode(img, distance=1.0, alpha_tree=alpha_tree, lf_tree=lf_tree)
    assert data != plain
    assert not plan_of([data])["lean_mod"] and plan_of([plain])["lean_mod"]
    batch(gpu_decoder, [data], taps=True)   # (with the stage taps on the pixel kernels run in another form, whose colour bytes differ by rounding: this decode is for the LF plane alone)
    for c in range(3):
        assert np.array_equal(gpu_decoder.read_plane(0, "lf_quant", c), plain_dump.planes["lf_quant"][c]), c
    got = batch(gpu_decoder, [data])[0]
    assert np.array_equal(got[..., 3], img[..., 3])
    assert got.tobytes() == plain_px.tobytes()
    strided = batch(gpu_decoder, [data], lane_stride=2)[0]
    assert strided.tobytes() == plain_px.tobytes()
    four = batch(gpu_decoder, [data, plain, data, data])
    assert all(f.tobytes() == plain_px.tobytes() for f in four)
