"""Modular transform lists on the CPU: the oracle's writer and reader (oracle_lib.encode(transforms=...), the `mod_coded` dump) held
against the numpy restatement of tests/transform_util.py, for every case of the table that tests/test_gpu_transform_chains.py then
decodes on the GPU.  Everything is exact; every case also proves that it exercises what its name says."""
import numpy as np
import pytest

import transform_util as TU


@pytest.fixture(scope="module")
def plain(oracle):
    """The file of each distinct picture without any transform."""
    memo = {}

    def get(case):
        key = (case.src.tobytes(), case.src.shape, case.bits)
        if key not in memo:
            memo[key] = case.encode(oracle, transforms=[])
        return memo[key]
    return get


@pytest.mark.parametrize("case", TU.CASES, ids=[c.name for c in TU.CASES])
def test_case_round_trip_and_restatement(oracle, plain, case):
    src = case.src
    h, w, nchan = src.shape
    data = case.encode(oracle)
    dec = oracle.decode(data, want_dump=True)
    assert dec.pixels.dtype == src.dtype and np.array_equal(dec.pixels, case.expected())
    coded = dec.planes["mod_coded"]
    # the channel list: count, order and sizes by the restatement's bookkeeping
    sizes, nb_meta, _ = TU.channel_list(nchan, w, h, case.transforms, case.colours)
    assert [c.shape for c in coded] == [(sh, sw) for sw, sh in sizes]
    assert nb_meta == sum(1 for t in case.transforms if t[0] == "palette")
    # the restatement's inverse of the coded channels is the picture
    back = TU.undo_transforms(coded, nchan, w, h, case.transforms)
    assert np.array_equal(np.stack(back, axis=2), src.astype(np.int64))
    # preconditions
    assert case.route == TU.route_of(case.transforms)
    assert data != plain(case), "the transform list left the file as it was"
    raw = oracle.decode(plain(case), want_dump=True).planes["mod_coded"]
    identity = all(t[0] == "rct" and t[2] == 0 for t in case.transforms)     # rct_type 0: no permutation, nothing added
    assert identity or len(raw) != len(coded) or any(not np.array_equal(a, b) for a, b in zip(raw, coded)), "the coded channels are the picture's own"
    flat = src.reshape(-1, nchan)
    assert case.colours == [1] or all(len(np.unique(flat[:, c])) > 1 for c in range(nchan)), "a flat channel hides what is done to it"
    if case.transforms[-1][0] == "rct":     # the three channels the last RCT left differ, so their order shows
        b = case.transforms[-1][1]          # (an index into the coded list: nothing behind it moves the channels)
        assert not any(np.array_equal(coded[b + i], coded[b + j]) for i, j in ((0, 1), (0, 2), (1, 2)))
    pal = [t for t in case.transforms if t[0] == "palette"]
    assert len(pal) == len(case.colours)
    if len(pal) == 1 and case.transforms[0][0] == "palette":
        _, b, n = pal[0]
        assert len(np.unique(flat[:, b:b + n], axis=0)) == case.colours[0]
    if len(pal) == 2:    # RGB, then alpha (behind one meta channel and the index channel)
        assert case.transforms[:2] == [("palette", 0, 3), ("palette", 2, 1)]
        assert [len(np.unique(flat[:, :3], axis=0)), len(np.unique(flat[:, 3]))] == case.colours
    if len(pal) == 1 and case.transforms[0][0] == "rct":   # a bijection in front keeps the count
        assert len(np.unique(flat, axis=0)) == case.colours[0]
        assert min(int(c.min()) for c in coded[:1]) < 0, "no negative palette entry"
    assert any(c.size == 0 for c in coded) == case.zero_size


def test_table_covers_both_routes():
    for route, least in TU.MIN_CASES.items():
        assert sum(1 for c in TU.CASES if c.route == route) >= least, route
    assert {c.route for c in TU.CASES} == set(TU.MIN_CASES)
    assert len({c.name for c in TU.CASES}) == len(TU.CASES)
    a = TU.cases_of("a")
    assert sorted(c.transforms[0][2] for c in a if c.route == "inline") == list(range(42))
    assert sorted(c.transforms[0][2] for c in a if c.transforms[-1] == ("squeeze", [])) == list(range(42))
    # the pair at the switch: the same list, cut to four
    by = {c.name: c for c in TU.CASES}
    assert by["chain4"].transforms == by["chain5"].transforms[:4] and (by["chain4"].route, by["chain5"].route) == ("inline", "launches")
    assert np.array_equal(by["chain4"].src, by["chain5"].src)


def test_permutation_table_is_a_set_of_permutations():
    assert len(set(TU.PERMUTATIONS)) == 6 and all(sorted(p) == [0, 1, 2] for p in TU.PERMUTATIONS)


@pytest.mark.parametrize("name,picture,transforms", TU.REFUSALS, ids=[r[0] for r in TU.REFUSALS])
def test_refusal_streams_are_refused_by_the_oracle(oracle, name, picture, transforms):
    data = oracle.encode(picture(), lossless=True, transforms=transforms)
    with pytest.raises(oracle.OracleError):
        oracle.decode(data)
    # the same list without its declared entry is a valid stream
    src = picture()
    assert np.array_equal(oracle.decode(oracle.encode(src, lossless=True, transforms=transforms[:-1])).pixels, src)


def test_transforms_keyword_limits(oracle):
    src = TU.rgb8(16, 8, 410)
    for kw in (dict(palette=True), dict(lossless_squeeze=True)):
        with pytest.raises(oracle.OracleError):
            oracle.encode(src, lossless=True, transforms=[("rct", 0, 6)], **kw)
    with pytest.raises(oracle.OracleError):
        oracle.encode(src, distance=1.0, transforms=[("rct", 0, 6)])
    with pytest.raises(oracle.OracleError):
        oracle.encode(src.astype(np.float32) / 255, lossless=True, float_samples=32, transforms=[("rct", 0, 6)])
    with pytest.raises(oracle.OracleError):     # a declared entry is the last one
        oracle.encode(src, lossless=True, transforms=[("declare", 0, 0, 6), ("rct", 0, 6)])
    with pytest.raises(oracle.OracleError):     # applied entries are checked
        oracle.encode(src, lossless=True, transforms=[("rct", 1, 6)])
    # the writer's own choice for RGB is the list [RCT 6]: the keyword reproduces its bytes, and the keyword left out changes nothing
    assert oracle.encode(src, lossless=True, transforms=[("rct", 0, 6)]) == oracle.encode(src, lossless=True)
    # a default Squeeze is written as a count of 0 (the writer's own lossless_squeeze spells the parameters out)
    own = oracle.encode(src, lossless=True, lossless_squeeze=True)
    short = oracle.encode(src, lossless=True, transforms=[("rct", 0, 6), ("squeeze", [])])
    assert len(short) < len(own)
    a, b = (oracle.decode(f, want_dump=True) for f in (own, short))
    assert np.array_equal(a.pixels, src) and np.array_equal(b.pixels, src)
    assert all(np.array_equal(x, y) for x, y in zip(a.planes["mod_coded"], b.planes["mod_coded"])) and len(a.planes["mod_coded"]) == len(b.planes["mod_coded"])


@pytest.mark.parametrize("w,h", [(1, 257), (1, 300), (1, 513), (1, 256), (1, 600), (300, 1)])
def test_one_pixel_wide_squeezed_frames_read_back(oracle, w, h):
    """Three channels, default Squeeze: the 0 x h residual channels of the 1-wide chroma channels are taller than a group, so the
    GlobalModular stream ends in front of them and the 1 x h/2 channels behind them travel in the groups (the reader used to skip
    the empty channels before it looked for the stream's end, and read those channels from the global stream)."""
    src = TU.rgb8(w, h, 420 + h)
    dec = oracle.decode(oracle.encode(src, lossless=True, lossless_squeeze=True), want_dump=True)
    assert np.array_equal(dec.pixels, src)
    coded = dec.planes["mod_coded"]
    assert any(c.size == 0 for c in coded)
    t = [("rct", 0, 6), ("squeeze", [])]
    assert np.array_equal(np.stack(TU.undo_transforms(coded, 3, w, h, t), axis=2), src)
