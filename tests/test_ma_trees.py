"""CPU tests of the explicit-tree writer of the oracle and of the tree families of ma_tree_util: every family at its sizes round-trips
through the oracle (the source pixels are the ground truth of a lossless codec), and the census of the paths the cases are built to
reach shows every label and every family."""
import numpy as np
import pytest

import ma_tree_util as M

CASES = M.families()


def test_census_shows_every_label_and_family(capsys):
    seen, by_family = {}, {}
    for c in CASES:
        labels = set()
        for w, h in c.sizes:
            labels |= M.census(c, w, h)
        assert labels <= set(M.LABELS)
        if c.expect:
            assert c.expect in labels, (c.id, labels)   # the case reaches what it was built for
        for l in labels:
            seen.setdefault(l, []).append(c.id)
        by_family.setdefault(c.family, set()).update(labels)
    with capsys.disabled():
        for f in M.FAMILIES:
            print("%-18s %s" % (f, " ".join(sorted(by_family.get(f, ())))))
    assert sorted(by_family) == sorted(M.FAMILIES)
    assert sorted(seen) == sorted(M.LABELS), seen.keys()
    used = {s for c in CASES for s in c.sizes}
    assert used >= set(M.SIZES)
    # the rows of the table that are a boundary of the decoder: one side stays on the grid, the other leaves it
    want = {"layout32/1 x 32": "grid-lanes", "layout32/1 x 33": "walk", "layout32/2 x 32": "grid-lds", "layout32/32 + 33": "walk",
            "layout16/3 props, 16": "grid-lds", "layout16/3 props, 17": "walk", "layout16/4 props, 16": "grid-lds", "layout16/4 props, 17": "walk",
            "cells/64": "grid-lanes", "cells/65": "grid-lds", "cells/2048": "grid-lds", "cells/4096": "walk", "> 4 properties/5 props": "walk"}
    for c in CASES:
        if c.id in want:
            assert {l for w, h in c.sizes for l in M.census(c, w, h)} == {want[c.id]}, c.id
    # one frame with a constant, a row-static and a per-sample channel
    mixed = next(c for c in CASES if c.family == "mixed classes")
    assert M.census(mixed, 130, 67) == {"const", "row-static", "grid-lanes"}
    # the stream-id case has channels in the global stream, in LF groups and in pass groups
    sid_case = next(c for c in CASES if c.name == "stream ids")
    (w, h), = sid_case.sizes
    sids = {s for s, _, _, _ in M.frame_streams(1, w, h, True)}
    nlf = -(-w // M.LF_GROUP_DIM)
    assert 0 in sids and any(nlf < s <= 2 * nlf for s in sids) and sum(s > 3 * nlf + M.K_NUM_QUANT_TABLES for s in sids) > 1
    # every property 2 .. 15 and every predictor occurs in a tree that reaches a grid, and in one that is walked
    for label in ("grid", "walk"):
        props, preds = set(), set()
        for c in CASES:
            for w, h in c.sizes:
                if any(l.startswith(label) for l in M.census(c, w, h)):
                    nodes = c.nodes(w, h)
                    props |= {n[0] for n in nodes if n[0] >= 0}
                    preds |= {n[4] for n in nodes if n[0] < 0}
        assert props >= set(range(2, 16)) and preds >= set(range(14)), (label, props, preds)


def test_classify_rules():
    """The restated rules on hand-made trees, one rule each."""
    f = M.flatten
    assert M.classify(f(M.L(5)), 0, 0, 9, 9) == "row-static"
    assert M.classify(f(M.L(0, 7)), 0, 0, 9, 9, one_symbol=[0]) == "const"
    assert M.classify(f(M.L(0, 7)), 0, 0, 9, 9) == "row-static"
    assert M.classify(f(M.L(3)), 0, 0, 9, 9) == "grid-lanes"                       # a predictor beyond 0, 1, 2, 5
    assert M.classify(f(M.S(2, 4, M.L(1), M.L(2))), 0, 0, 9, 9) == "row-static"
    assert M.classify(f(M.S(2, 4, M.L(1), M.L(7))), 0, 0, 9, 4) == "grid-lanes"    # row 0 already ends in predictor 7
    assert M.classify(f(M.S(2, 4, M.L(7), M.L(1))), 0, 0, 9, 5) == "row-static"    # rows 0 .. 4 only
    assert M.classify(f(M.S(2, 4, M.L(7), M.L(1))), 0, 0, 9, 6) == "grid-lanes"
    assert M.classify(f(M.S(0, 0, M.L(6), M.L(1))), 0, 0, 9, 9) == "grid-lanes"    # the weighted predictor somewhere in the tree
    assert M.classify(f(M.S(2, 60, M.L(5), M.L(1))), 0, 0, M.K_CARRY_INTS + 1, 65) != "row-static"
    assert M.classify(f(M.S(2, 60, M.L(5), M.L(1))), 0, 0, M.K_CARRY_INTS, 65) == "row-static"


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_family_round_trips_through_the_oracle(oracle, case):
    for w, h in case.sizes:
        src = case.image(w, h)
        nodes = case.nodes(w, h)
        assert len(nodes) < 1024   # below the size limit of a tree whatever the frame size
        data = oracle.encode(src, tree=nodes, **case.encode_args())
        got = oracle.decode(data).pixels
        assert got.dtype == src.dtype and got.tobytes() == src.tobytes(), (w, h)
        assert data != oracle.encode(src, **case.encode_args())   # the tree was really used


def test_multiplier_needs_matching_residuals(oracle):
    """The tokeniser refuses a residual that its leaf's multiplier does not divide (nothing is rounded silently)."""
    src = np.arange(12, dtype=np.uint8).reshape(3, 4, 1) * 2 + 1
    with pytest.raises(oracle.OracleError):
        oracle.encode(src, lossless=True, tree=M.flatten(M.L(0, 0, 2)))
    data = oracle.encode(src, lossless=True, tree=M.flatten(M.L(0, 1, 2)))
    assert np.array_equal(oracle.decode(data).pixels, src)
    for bad in ([[3, 0, 1, 1, 0, 0, 1]], [[-1, 0, 0, 0, 14, 0, 1]], [[-1, 0, 0, 0, 0, 0, 0]], [[16, 0, 1, 2, 0, 0, 1], [-1, 0, 0, 0, 0, 0, 1], [-1, 0, 0, 0, 0, 0, 1]]):
        with pytest.raises(oracle.OracleError):
            oracle.encode(src, lossless=True, tree=bad)


def test_lossy_frames_take_alpha_and_lf_trees(oracle):
    """A tree changes the coding of a lossy frame, not its content."""
    from pdn_jpegxl_amd.synth import synth
    img = synth(130, 67, 5)
    plain = oracle.encode(img)
    ref = oracle.decode(plain, want_dump=True)
    for kw in (dict(alpha_tree=M.flatten(M.buckets(10, [-2, 0, 6], [M.L(5), M.L(4), M.L(7), M.L(1)]))),
               dict(lf_tree=M.flatten(M.nest([(15, [-9, 0, 8])], M.Leaves([6])))),
               dict(alpha_tree=M.flatten(M.L(2)), lf_tree=M.flatten(M.buckets(9, [-3, 0, 3], [M.L(q) for q in (1, 5, 12, 13)])))):
        data = oracle.encode(img, **kw)
        assert data != plain
        got = oracle.decode(data, want_dump=True)
        assert np.array_equal(got.pixels, ref.pixels)
        assert all(np.array_equal(a, b) for a, b in zip(got.planes["lf_quant"], ref.planes["lf_quant"]))
        assert np.array_equal(got.planes["alpha"], ref.planes["alpha"])
