"""CPU checks of the Modular sample rules that every decode loop, the lossless encoder's kernels and its host code call
(csrc/modular_rules.h), through the jxlhip_selftest_* exports of csrc/selftest.cc.  Each rule is held against the format's definition
written out here independently, in Python's unbounded integers."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ma_tree_util as T
from pdn_jpegxl_amd import api

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
VALUES = [0, 1, -1, 2, -2, 255, -255, 65535, -65535, I32_MIN, I32_MAX]
M32 = (1 << 32) - 1


def _lib():
    return api.selftest_lib()


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def tdiv(a, b):
    """Division truncating toward zero, as the format's integer arithmetic divides."""
    q = abs(a) // b
    return -q if a < 0 else q


def s32(v):
    """The low 32 bits of v as a signed number."""
    v &= M32
    return v - (1 << 32) if v >> 31 else v


# ---------------------------------------------------------------- the format's definitions
def predict(p, W, N, NW, NE, NN, WW, NEE, wp):
    if p == 0:
        return 0
    if p == 1:
        return W
    if p == 2:
        return N
    if p == 3:
        return tdiv(W + N, 2)
    if p == 4:
        g = W + N - NW
        return W if abs(g - W) < abs(g - N) else N
    if p == 5:
        return max(min(W, N), min(max(W, N), W + N - NW))
    if p == 6:
        return wp
    if p == 7:
        return NE
    if p == 8:
        return NW
    if p == 9:
        return WW
    if p == 10:
        return tdiv(W + NW, 2)
    if p == 11:
        return tdiv(N + NW, 2)
    if p == 12:
        return tdiv(N + NE, 2)
    return tdiv(6 * N - 2 * NN + 7 * W + WW + NEE + 3 * NE + 8, 16)


def prop(i, W, N, NW, NE, NN, WW, x, y, prev9, wp_err):
    return {2: y, 3: x, 4: abs(N), 5: abs(W), 6: N, 7: W, 8: W - prev9, 9: W + N - NW, 10: W - NW, 11: NW - N, 12: N - NE,
            13: N - NN, 14: W - WW, 15: wp_err}[i]


def hood_at(img, x, y):
    """(W, N, NW, NE, NN, WW, NEE) of sample (x, y) by the definition, img[y][x]."""
    h, w = len(img), len(img[0])
    W = img[y][x - 1] if x else (img[y - 1][0] if y else 0)
    N = img[y - 1][x] if y else W
    NW = img[y - 1][x - 1] if x and y else W
    NE = img[y - 1][x + 1] if y and x + 1 < w else N
    NN = img[y - 2][x] if y > 1 else N
    WW = img[y][x - 2] if x > 1 else W
    NEE = img[y - 1][x + 2] if y and x + 2 < w else NE
    return W, N, NW, NE, NN, WW, NEE


# ---------------------------------------------------------------- inputs shared by the predictor and the property tests
@pytest.fixture(scope="module")
def hoods():
    """Every triple of VALUES as (W, N, NW), as (NE, NN, WW) and as (NEE, N, W), the other neighbours taken from the same triple in
    another order (so the inputs of predictors 7, 9, 12 and 13 see every triple too), and 2000 seeded random neighbourhoods."""
    rows = []
    for a, b, c in itertools.product(VALUES, repeat=3):
        rows.append((a, b, c, c, a, b, b))
        rows.append((c, a, b, a, b, c, a))
        rows.append((c, b, a, b, c, a, a))
    rng = np.random.default_rng(20240607)
    wide = rng.integers(I32_MIN, I32_MAX, size=(1000, 7), endpoint=True)
    near = rng.integers(-300, 300, size=(1000, 7), endpoint=True)
    rows += [tuple(int(v) for v in r) for r in np.concatenate([wide, near])]
    arr = np.ascontiguousarray(np.array(rows, dtype=np.int32))
    n = len(rows)
    extra = np.random.default_rng(7)
    wp = extra.integers(-(1 << 34), 1 << 34, size=n).astype(np.int64)          # the weighted prediction / property 15
    prev9 = extra.integers(-(1 << 33), 1 << 33, size=n).astype(np.int64)
    xy = np.ascontiguousarray(extra.integers(0, 1 << 20, size=(n, 2)).astype(np.int32))
    return rows, arr, wp, prev9, xy


def test_predictors_equal_the_definition_in_the_low_32_bits(hoods):
    rows, arr, wp, _, _ = hoods
    n = len(rows)
    by_id = np.zeros((n, 14), np.int32)
    by_t = np.zeros((n, 14), np.int32)
    g32 = np.zeros(n, np.int32)
    rg = np.zeros((n, 4), np.uint32)
    _lib().jxlhip_selftest_modular_predict(C.c_int32(n), _p(arr, C.c_int32), _p(wp, C.c_int64), _p(by_id, C.c_int32), _p(by_t, C.c_int32),
                                            _p(g32, C.c_int32), _p(rg, C.c_uint32))
    want = np.array([[s32(predict(p, *r, int(wp[i]))) for p in range(14)] for i, r in enumerate(rows)], dtype=np.int64)
    assert np.array_equal(by_id.astype(np.int64), want)
    assert np.array_equal(by_t.astype(np.int64), want)
    assert np.array_equal(g32.astype(np.int64), want[:, 5])                    # ClampedGradient32 is predictor 5
    assert np.array_equal(rg.astype(np.int64), want[:, [0, 1, 2, 5]] & M32)    # RowGuess: 0, 1, 2, 5


def test_properties_and_their_linear_forms_agree_with_the_definition(hoods):
    rows, arr, wp, prev9, xy = hoods
    n = len(rows)
    out = np.zeros((n, 14), np.int64)
    _lib().jxlhip_selftest_modular_property(C.c_int32(n), _p(arr, C.c_int32), _p(prev9, C.c_int64), _p(wp, C.c_int64), _p(xy, C.c_int32),
                                             _p(out, C.c_int64))
    forms = {}
    for i in range(2, 16):
        f = np.zeros(11, np.int32)
        _lib().jxlhip_selftest_modular_property_form(C.c_int32(i), _p(f, C.c_int32))
        forms[i] = [int(v) for v in f]
        assert set(forms[i][:9]) <= {-1, 0, 1} and set(forms[i][9:]) <= {0, 1}
    for k, (W, N, NW, NE, NN, WW, _) in enumerate(rows):
        x, y, p9, e = int(xy[k, 0]), int(xy[k, 1]), int(prev9[k]), int(wp[k])
        for i in range(2, 16):
            want = prop(i, W, N, NW, NE, NN, WW, x, y, p9, e)
            assert int(out[k, i - 2]) == want, (i, rows[k])
            f = forms[i]
            v = sum(c * t for c, t in zip(f[:9], (W, N, NW, NE, NN, WW, x, y, e))) - p9 * f[10]
            assert (abs(v) if f[9] else v) == want, (i, rows[k])   # what the grid's lanes evaluate is what the walk tests


@pytest.mark.parametrize("w,h", [(1, 1), (4, 1), (1, 4), (2, 2), (5, 3)])
def test_neighbourhood_by_roll_and_by_position_equal_direct_indexing(w, h):
    img = np.ascontiguousarray(np.random.default_rng(100 * w + h).integers(-1000, 1000, size=(h, w)).astype(np.int32))
    rows = [[int(v) for v in r] for r in img]
    want_h, want_p = [], []
    for y in range(h):
        for x in range(w):
            want_h.append(hood_at(rows, x, y))
            if x:
                pw, pn, pnw = hood_at(rows, x - 1, y)[:3]
                want_p.append(pw + pn - pnw)
            else:
                want_p.append(0)
    for by_roll in (1, 0):
        got_h = np.zeros((h * w, 7), np.int32)
        got_p = np.zeros(h * w, np.int64)
        _lib().jxlhip_selftest_modular_hoods(C.c_int32(w), C.c_int32(h), _p(img, C.c_int32), C.c_int32(by_roll), _p(got_h, C.c_int32),
                                              _p(got_p, C.c_int64))
        assert [tuple(int(v) for v in r) for r in got_h] == want_h, by_roll
        assert [int(v) for v in got_p] == want_p, by_roll


def test_signed_packing_round_trips_and_orders_by_magnitude():
    pack, unpack = _lib().jxlhip_selftest_pack_signed, _lib().jxlhip_selftest_unpack_signed
    pack.restype, pack.argtypes = C.c_uint32, [C.c_int32]
    unpack.restype, unpack.argtypes = C.c_int32, [C.c_uint32]
    for v in VALUES + list(range(-40, 40)) + [I32_MIN + 1, I32_MAX - 1]:
        want = 2 * v if v >= 0 else -2 * v - 1
        assert pack(v) == want & M32
        assert unpack(want & M32) == v


def test_one_symbol_token_for_every_flag_split_and_symbol():
    f = _lib().jxlhip_selftest_one_symbol_token
    f.restype, f.argtypes = C.c_int32, [C.c_uint32]
    for flag in (0, 1):
        for split in range(16):
            for msb_lsb in (0, 0x21 << 4):   # the other fields of the word do not matter
                # 0 .. 255: every ANS symbol; the larger ones: what a prefix code's single symbol may be (the whole upper half-word)
                syms = list(range(256)) + [256, 300, 511, 512, 32767, 32768, 40000, 65535]
                got = [f(split | msb_lsb | flag << 12 | sym << 16) for sym in syms]
                assert got == [sym if flag and sym < (1 << split) else -1 for sym in syms], (flag, split)


def test_leaf_residual_wraps_like_the_low_half_of_the_wide_product():
    f = _lib().jxlhip_selftest_leaf_residual
    f.restype, f.argtypes = C.c_uint32, [C.c_uint32] * 3
    tokens = [0, 1, 2, 3, 4, 255, 256, 65535, (1 << 31) - 1, 1 << 31, M32 - 1, M32]
    for mul in (1, 2, 96, (1 << 31) - 1, M32):
        for off in (0, 1, -1, I32_MIN):
            for u in tokens:
                signed = u >> 1 if not u & 1 else -((u + 1) >> 1)
                assert f(u, mul, off & M32) == (signed * mul + off) & M32, (u, mul, off)


@pytest.mark.parametrize("tree", [T._row_tree, T._sid_tree, T._static_tree], ids=["row", "sid", "static"])
def test_static_walk_ends_where_the_restated_walk_ends(tree):
    walk = _lib().jxlhip_selftest_static_walk
    walk.restype = C.c_int32
    for w, h in T.SIZES:
        nodes = T.flatten(tree(w, h))
        # leaves as the decoder holds them: offset, predictor | context << 8 (the context here: the node's own index), multiplier
        dev = np.ascontiguousarray(np.array([[n[0], n[1], n[2], n[3]] if n[0] >= 0 else [-1, n[5], n[4] | i << 8, n[6]]
                                             for i, n in enumerate(nodes)], dtype=np.int32))
        sids = sorted({sid for sid, _, _, _ in T.frame_streams(1, w, h, True)})
        for chan in (0, 1, 2):
            for sid in sids:
                for y in range(h):
                    out = np.zeros(3, np.int32)
                    got = walk(_p(dev, C.c_int32), C.c_int32(len(nodes)), C.c_int32(chan), C.c_int32(sid), C.c_int32(y), C.c_int32(1),
                               _p(out, C.c_int32))
                    want, used_y = T._row_leaf(nodes, chan, sid, y)
                    assert (got, bool(out[0])) == (want, used_y), (w, h, chan, sid, y)
                    if nodes[want][0] < 0:
                        assert (int(out[1]), int(out[2])) == (nodes[want][4], want)
                # channel and stream only: the walk stops at the first node that tests anything else, the row included
                i = 0
                while 0 <= nodes[i][0] <= 1:
                    i = nodes[i][2] if (chan, sid)[nodes[i][0]] > nodes[i][1] else nodes[i][3]
                out = np.zeros(3, np.int32)
                assert walk(_p(dev, C.c_int32), C.c_int32(len(nodes)), C.c_int32(chan), C.c_int32(sid), C.c_int32(0), C.c_int32(0),
                            _p(out, C.c_int32)) == i and not out[0]


def wp_model(img):
    """The format's weighted predictor with its default parameters, memory form: per row parity the true errors and the four
    sub-predictor errors, w + 2 entries each; returns per sample (prediction, property 15)."""
    h, w = len(img), len(img[0])
    err = [[0] * (w + 2) for _ in range(2)]
    sub_err = [[[0] * (w + 2) for _ in range(2)] for _ in range(4)]
    maxw = (13, 12, 12, 12)

    def div(i):
        return (1 << 24) // (i + 1)

    def weight(x, m):
        shift = max((x + 1).bit_length() - 1 - 5, 0)
        return 4 + ((m * div(x >> shift)) >> shift)

    out = []
    for y in range(h):
        cur, prev = (0, 1) if y & 1 else (1, 0)
        for x in range(w):
            W, N, _, NE = hood_at(img, x, y)[:4]
            xn, xne, xnw = x, (x + 1 if x < w - 1 else x), (x - 1 if x > 0 else x)
            wts = [weight(sub_err[i][prev][xn] + sub_err[i][prev][xne] + sub_err[i][prev][xnw], maxw[i]) for i in range(4)]
            W8, N8, NE8 = W * 8, N * 8, NE * 8
            te_w = err[cur][x - 1] if x else 0
            te_n, te_nw, te_ne = err[prev][xn], err[prev][xnw], err[prev][xne]
            max_err = te_w
            for t in (te_n, te_nw, te_ne):
                if abs(t) > abs(max_err):
                    max_err = t
            sub = [W8 + NE8 - N8,
                   N8 - (((te_w + te_n + te_ne) * 16) >> 5),
                   W8 - (((te_w + te_n + te_nw) * 10) >> 5),
                   N8 - ((te_nw * 7 + te_n * 7 + te_ne * 7) >> 5)]
            log_weight = sum(wts).bit_length() - 1
            wts = [v >> (log_weight - 4) for v in wts]
            total = sum(wts)
            s = (total >> 1) - 1 + sum(p * v for p, v in zip(sub, wts))
            pred = (s * div(total - 1)) >> 24
            if ((te_n ^ te_w) | (te_n ^ te_nw)) <= 0:
                pred = max(min(W8, N8, NE8), min(max(W8, N8, NE8), pred))
            out.append(((pred + 3) >> 3, max_err))
            v8 = img[y][x] * 8
            err[cur][x] = pred - v8
            for i in range(4):
                e = (abs(sub[i] - v8) + 3) >> 3
                sub_err[i][cur][x] = e
                sub_err[i][prev][x + 1] += e
    return out


@pytest.mark.parametrize("w,h", [(1, 1), (5, 1), (1, 5), (2, 2), (7, 5), (33, 4)])
def test_weighted_predictor_equals_the_memory_form_model(w, h):
    run = _lib().jxlhip_selftest_wp
    for k, (lo, hi) in enumerate([(0, 1 << 8), (0, 1 << 16), (-(1 << 20), 1 << 20)]):
        rng = np.random.default_rng(1000 * w + 10 * h + k)
        img = rng.integers(lo, hi, size=(h, w))
        if k == 1 and w > 2:
            img[:, w // 2:] = img[:, :1] + rng.integers(-2, 3, size=(h, w - w // 2))   # a flat half: small errors, large weights
        img = np.ascontiguousarray(img.astype(np.int32))
        guess = np.zeros(h * w, np.int64)
        max_err = np.zeros(h * w, np.int64)
        run(C.c_int32(w), C.c_int32(h), _p(img, C.c_int32), _p(guess, C.c_int64), _p(max_err, C.c_int64))
        want = wp_model([[int(v) for v in r] for r in img])
        assert [(int(g), int(e)) for g, e in zip(guess, max_err)] == want, (w, h, lo, hi)
