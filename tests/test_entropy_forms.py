"""The entropy-code forms of tests/entropy_forms_util.py on the CPU: the oracle round-trips every stream, the knob changes nothing but the
coding (every dumped plane is byte-identical to the dump of the same call without entropy=, which never passes through the code under
test), the census shows what each case is built to reach, and the product's parser accepts the file."""
import pytest

import entropy_forms_util as EU
from pdn_jpegxl_amd import api

PLANES = ("qcoef", "lf_quant", "alpha", "strategy", "raw_quant", "sharpness", "ytox", "ytob", "mod_coded")


def same_dumps(a, b):
    for name in PLANES:
        pa, pb = a.planes[name], b.planes[name]
        if isinstance(pa, list):
            assert len(pa) == len(pb) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(pa, pb)), name
        else:
            assert pa.dtype == pb.dtype and pa.tobytes() == pb.tobytes(), name


@pytest.mark.parametrize("case", EU.CASES, ids=[c.id for c in EU.CASES])
def test_case_round_trips_and_reaches_its_form(oracle, case):
    src = case.picture()
    data = case.encode(oracle)
    cen = oracle.entropy_census()
    plain = case.encode(oracle, entropy=False)
    assert data != plain
    got, ref = oracle.decode(data, want_dump=True), oracle.decode(plain, want_dump=True)
    assert got.pixels.dtype == ref.pixels.dtype and got.pixels.tobytes() == ref.pixels.tobytes()
    if case.lossless:
        assert got.pixels.tobytes() == src.tobytes()
    same_dumps(got, ref)
    case.check(cen)
    status, _, message = api.parse_check(data)
    assert status == "Ok", (status, message)


def test_defaults_keep_every_byte(oracle):
    """entropy={} (and lz={} beside lz77=True) writes the stream of the call without it."""
    rgb = EU.noise(40, 24, 3, 1)
    flat = EU.runs(40, 24, 9, 2)
    rgba = EU.synth(64, 64, 3)
    assert oracle.encode(rgb, lossless=True, entropy={}) == oracle.encode(rgb, lossless=True)
    assert oracle.encode(flat, lossless=True, entropy=dict(lz={})) == oracle.encode(flat, lossless=True, lz77=True)
    assert oracle.encode(rgba, entropy={}) == oracle.encode(rgba)
    assert oracle.encode(rgba, entropy=dict(lz={}), prefix_codes=True) == oracle.encode(rgba, lz77=True, prefix_codes=True)
    assert oracle.encode(rgba, entropy=dict(cfgs=[(4, 2, 0)]), wide_codes=True) == oracle.encode(rgba, wide_codes=True)


def test_special_distance_table(oracle):
    """The oracle's 120 pairs are distinct and are exactly dy = 0, dx = 1..8 and dy = 1..7, dx = -7..8; the case table's copy, written
    out on its own, agrees with them row by row."""
    table = oracle.special_distances()
    want = {(dx, 0) for dx in range(1, 9)} | {(dx, dy) for dy in range(1, 8) for dx in range(-7, 9)}
    assert len(table) == 120 and len(set(table)) == 120 and set(table) == want
    assert table == EU.SPECIAL
    assert sorted(k for f in EU.SPECIAL_FILES for k in f) == list(range(120))


def test_oracle_reader_uses_the_table_by_index(oracle):
    """One index per stream: a picture that repeats at (dx, dy) alone, written with that index only, must come back."""
    for k in range(120):
        src = EU.banded(20, 9, [EU.SPECIAL[k]], 300 + k)
        data = oracle.encode(src, lossless=True, tree=EU.ZERO_TREE, entropy=dict(lz=dict(distances=[k])))
        assert oracle.entropy_census()["special"][k] >= 1, k
        assert oracle.decode(data).pixels.tobytes() == src.tobytes(), k


def test_invalid_requests_are_oracle_errors(oracle):
    rgb = EU.noise(33, 17, 3, 4)
    small = EU.noise(40, 24, 1, 14, 16)   # every token below 32 under these configurations: log_alpha 5
    for bad in (dict(cfgs=[(6, 0, 0)]), dict(cfgs=[(5, 2, 1)])):
        with pytest.raises(oracle.OracleError):
            oracle.encode(small, lossless=True, tree=EU.ZERO_TREE, entropy=bad)
    for bad in (dict(cfgs=[(4, 5, 0)]), dict(cfgs=[(4, 2, 3)]), dict(hist=("shift", 14)),
                dict(hist="other"), dict(nothing=1), dict(lz=dict(distances=[120])), dict(lz=dict(len_cfg=(9, 0, 0)))):
        with pytest.raises(oracle.OracleError):
            oracle.encode(rgb, lossless=True, entropy=bad)
    with pytest.raises(oracle.OracleError):   # tokens reach 256 without prefix codes
        oracle.encode(rgb, lossless=True, wide_codes=True, entropy=dict(cfgs=[(8, 0, 0)]))
    # a failed call leaves no forms behind
    assert oracle.encode(rgb, lossless=True) == oracle.encode(rgb, lossless=True, entropy={})


@pytest.mark.parametrize("name,entropy,enc", EU.REFUSALS, ids=[r[0] for r in EU.REFUSALS])
def test_invalid_headers_are_refused_with_a_message(oracle, name, entropy, enc):
    data = oracle.encode(EU.noise(33, 17, 3, 5), lossless=True, entropy=entropy, **enc)
    with pytest.raises(oracle.OracleError) as e:
        oracle.decode(data)
    assert len(str(e.value)) > 4
    status, _, message = api.parse_check(data)
    assert status != "Ok" and len(message) > 4, (status, message)


def test_corrupt_variants_are_what_they_are_meant_to_be(oracle):
    """The intact stream decodes; of the damaged ones at least one length flip and the cut are errors, at least one distance flip decodes
    to other pixels (extra bits are not covered by the ANS state), and none of them decodes to the source by another route than the
    clamp (distance bit 0: 14 back with 13 values decoded is 13 back)."""
    src, data, variants = EU.corrupt_variants(oracle)
    assert oracle.decode(data).pixels.tobytes() == src.tobytes()
    verdict = {}
    for name, bad in variants:
        assert bad != data and len(bad) <= len(data)
        try:
            verdict[name] = int((oracle.decode(bad).pixels != src).sum())
        except oracle.OracleError as e:
            assert len(str(e)) > 4
            verdict[name] = "error"
    assert verdict["truncated"] == "error" and verdict["length bit 0"] == "error", verdict
    assert verdict["distance bit 0"] == 0 and isinstance(verdict["distance bit 2"], int) and verdict["distance bit 2"] > 0, verdict
