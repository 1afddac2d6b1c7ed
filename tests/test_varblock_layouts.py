"""Varblock layouts chosen by the test (CPU side): the oracle's writer and reader against the numpy restatement of the placement rule,
the writer's soundness against the source picture, the layouts a decoder must refuse, and the census of the case table that
tests/test_gpu_varblock_layouts.py decodes on the GPU."""
import numpy as np
import pytest

import varblock_util as V


def encode_case(oracle, case, **kw):
    return oracle.encode(V.smooth(case.w, case.h), distance=1.0, varblocks=case.blocks, **kw)


@pytest.fixture(scope="module")
def decoded(oracle):
    """Each valid case written and read back by the oracle once."""
    return {c.name: oracle.decode(encode_case(oracle, c), want_dump=True) for c in V.CASES}


# ---------------------------------------------------------------- the table itself
def test_case_table_census():
    """What the table must keep covering, so that a later edit cannot thin it unnoticed."""
    total = dict(misaligned={}, crosses_tile=False, crosses_cfl_tile=False, touches_partial_tile=False, pairs_v=set(), pairs_h=set())
    for c in V.CASES:
        assert c.w <= 272 and c.h <= 272, c
        cen = V.census(c.plane)
        for s, classes in cen["misaligned"].items():
            total["misaligned"].setdefault(s, set()).update(classes)
        for k in ("crosses_tile", "crosses_cfl_tile", "touches_partial_tile"):
            total[k] = total[k] or cen[k]
        total["pairs_v"] |= cen["pairs_v"]
        total["pairs_h"] |= cen["pairs_h"]
    for s in V.MULTI_CELL:
        assert total["misaligned"].get(s, set()) == V.allowed_classes(s), V.NAMES[s]
    assert total["crosses_tile"] and total["crosses_cfl_tile"] and total["touches_partial_tile"]
    every = {(a, b) for a in (3, 4, 5, 6) for b in (3, 4, 5, 6)}
    assert total["pairs_v"] == every and total["pairs_h"] == every


def test_named_cases():
    n = V.BY_NAME
    assert V.generic_tiles(n["tile-corner-64"].plane) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert V.gemm_tiles(n["tile-corner-64"].plane) == []                    # no tile lies wholly inside the block
    big = n["big-128"].plane
    assert len(V.generic_tiles(big)) == 9 and V.gemm_tiles(big) == [(1, 1)]   # tile (2, 2) holds one cell of the block: not a matrix-core tile
    # aligned layouts: nothing for the generic kernels, and exactly the length pairs an aligned layout can show
    al = n["aligned-pairs"].plane
    cen = V.census(al)
    assert V.generic_tiles(al) == [] and not cen["misaligned"]
    assert cen["pairs_v"] == V.ALIGNED_PAIRS and cen["pairs_h"] == V.ALIGNED_PAIRS
    # tile-interior: no block leaves its tile and none is special, so exactly the three tiles with shifted blocks are listed
    ti = n["tile-interior"].plane
    assert V.generic_tiles(ti) == [(0, 0), (0, 1), (1, 0)] and not V.census(ti)["crosses_tile"]
    assert not any(s in V.SPECIAL for s, _, _ in V.blocks_of(ti))
    # small-shifts: specials beside the shifted blocks, a 16x16 in four tiles
    ss = n["small-shifts"]
    assert (V.S["DCT16X16"], 7, 7) in V.blocks_of(ss.plane)
    used = {s for s, _, _ in V.blocks_of(ss.plane)}
    assert set(V.SPECIAL) <= used


def test_split_rows_cuts_rows_into_runs():
    c = V.BY_NAME["split-rows"]
    seq = [(s, 16) for s, _, _ in V.blocks_of(c.plane)]
    rows = V.free_runs(seq, c.w8, c.h8)
    assert sum(len(r) >= 3 for r in rows) >= 4, [len(r) for r in rows]
    # below the first row: a run of free cells that spans cells 31 and 32, i.e. ends at bit 31 of one coverage word and goes on at bit 0
    # of the next; and runs that end or start there on their own
    spans = ends = starts = 0
    for r in rows[1:]:
        if len(r) < 2:
            continue
        spans += any(x0 <= 31 and x0 + n > 32 for x0, n in r)
        ends += any(x0 + n == 32 for x0, n in r)
        starts += any(x0 == 32 for x0, n in r)
    assert spans >= 1 and ends >= 1 and starts >= 1, (spans, ends, starts)


# ---------------------------------------------------------------- the oracle's reader against the numpy rule
@pytest.mark.parametrize("case", V.CASES, ids=repr)
def test_oracle_places_blocks_as_the_rule_says(decoded, case):
    od = decoded[case.name]
    assert (od.w8, od.h8) == (case.w8, case.h8)
    strategy = od.planes["strategy"].reshape(case.h8, case.w8)
    raw_quant = od.planes["raw_quant"].reshape(case.h8, case.w8)
    assert np.array_equal(strategy, case.plane)                      # the writer put every block where the case says
    for s, bx, by, q in case.blocks:
        assert (raw_quant[by:by + V.COVERED_Y[s], bx:bx + V.COVERED_X[s]] == q).all()
    # the coded sequence, placed by the numpy rule, gives both planes back
    plane, quant = V.place(V.coding_order(strategy, raw_quant), case.w8, case.h8)
    assert np.array_equal(plane, strategy) and np.array_equal(quant, raw_quant)


# ---------------------------------------------------------------- writer soundness against the source picture
@pytest.mark.parametrize("case", V.CASES, ids=repr)
def test_writer_soundness(oracle, decoded, case):
    """The decode of a chosen layout is as close to the source as the DCT8-only encode of the same picture: over the whole picture up to
    MAX_ERROR_RATIO, over each named multi-cell block up to MAX_BLOCK_ERROR_RATIO (varblock_util: where the bounds come from)."""
    src = V.smooth(case.w, case.h)[..., :3].astype(np.float64)
    base = np.abs(oracle.decode(oracle.encode(V.smooth(case.w, case.h), distance=1.0, strategy_mode=1)).pixels[..., :3] - src)
    got = np.abs(decoded[case.name].pixels[..., :3] - src)
    worst = 0.0
    for s, bx, by, _ in case.blocks:
        cx, cy = V.COVERED_X[s], V.COVERED_Y[s]
        if cx * cy > 1:
            region = (slice(by * 8, (by + cy) * 8), slice(bx * 8, (bx + cx) * 8))
            worst = max(worst, got[region].mean() / max(0.25, base[region].mean()))
    print("%s: mean abs error %.3f, DCT8 only %.3f, ratio %.2f, worst block %.2f" % (case.name, got.mean(), base.mean(), got.mean() / base.mean(), worst))
    assert got.mean() <= V.MAX_ERROR_RATIO * base.mean(), (got.mean(), base.mean())
    assert worst <= V.MAX_BLOCK_ERROR_RATIO, worst


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("name,w,h,seq,reason", V.INVALID, ids=[i[0] for i in V.INVALID])
def test_invalid_sequences_are_refused(oracle, name, w, h, seq, reason):
    with pytest.raises(V.LayoutError) as e:
        V.place(seq, (w + 7) // 8, (h + 7) // 8)
    assert str(e.value) == reason
    data = oracle.encode(V.smooth(w, h), varblock_sequence=seq)
    with pytest.raises(oracle.OracleError) as e:
        oracle.decode(data)
    assert reason in str(e.value)


def test_valid_sequence_round_trips(oracle):
    """varblock_sequence itself is sound: the valid sequence the refusal cases are cut from decodes to the layout the rule gives."""
    name, w, h, seq, _ = [i for i in V.INVALID if i[0] == "count-long"][0]
    seq = seq[:-1]
    plane, quant = V.place(seq, 4, 3)
    od = oracle.decode(oracle.encode(V.smooth(w, h), varblock_sequence=seq), want_dump=True)
    assert np.array_equal(od.planes["strategy"].reshape(3, 4), plane)
    assert np.array_equal(od.planes["raw_quant"].reshape(3, 4), quant)


@pytest.mark.parametrize("blocks", [
    [(V.S["DCT16X16"], 1, 1), (V.S["DCT8X16"], 2, 2)],      # overlap
    [(V.S["DCT8X16"], 31, 0)],                              # crosses the group edge in x
    [(V.S["DCT16X8"], 0, 31)],                              # ... in y
    [(V.S["DCT8X32"], 31, 4)],                              # leaves the frame
    [(V.S["DCT16X16"], -1, 0)],
    [(27, 0, 0)], [(V.S["AFV0"], 0, 0)],
], ids=["overlap", "group-x", "group-y", "frame", "negative", "unknown", "afv"])
def test_writer_rejects_bad_varblocks(oracle, blocks):
    with pytest.raises(oracle.OracleError):
        oracle.encode(V.smooth(272, 272), varblocks=blocks)
