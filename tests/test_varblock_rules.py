"""CPU checks of the varblock rules that the decoder's placement and reconstruction kernels, the encoder's front end and the host all
call (csrc/varblock_rules.h), and of recon_tile_kernel's LDS layout (csrc/lds_layout.h), through the jxlhip_selftest_varblock_* exports
of csrc/selftest.cc.  Each rule is held against a statement written out here."""
import ctypes as C

import numpy as np
import pytest

import varblock_util as V
from pdn_jpegxl_amd import api

AFV = [V.S["AFV0"], V.S["AFV1"], V.S["AFV2"], V.S["AFV3"]]


def _lib():
    lib = api.selftest_lib()
    lib.jxlhip_selftest_varblock_dequant_bias.restype = C.c_float
    lib.jxlhip_selftest_varblock_dequant_bias.argtypes = [C.c_int32, C.c_float, C.c_float, C.c_int32]
    lib.jxlhip_selftest_varblock_cell_pack.restype = C.c_uint32
    lib.jxlhip_selftest_varblock_cell_pack.argtypes = [C.c_uint32] * 5
    return lib


def _strategy(lib, s):
    out = (C.c_int32 * 6)()
    lib.jxlhip_selftest_varblock_strategy(C.c_int32(s), out)
    return list(out)


def _unpack(lib, info):
    out = (C.c_uint32 * 7)()
    lib.jxlhip_selftest_varblock_cell_unpack(C.c_uint32(info), out)
    return list(out)


def _dims(name):
    """(rows, columns) in samples from a strategy's name; the 8x8 transforms without a plain DCT have one cell."""
    if name.startswith("DCT") and "X" in name:
        r, c = name[3:].split("X")
        return max(int(r), 8), max(int(c), 8)
    return 8, 8


# ---------------------------------------------------------------- tables
def test_strategy_tables():
    lib = _lib()
    # order buckets and quant tables from the names: numbered in order of first appearance; a shape and its transpose share both;
    # IDENTITY, DCT2X2 and DCT4X4 share bucket 1 with the other special 8x8 transforms but have tables of their own
    want_bucket, want_table = [], []
    buckets, tables = {}, {}
    for s, name in enumerate(V.NAMES):
        r, c = _dims(name)
        special = s in V.SPECIAL or s in AFV
        bkey = "special" if special else (max(r, c), min(r, c))
        tkey = name if name in ("IDENTITY", "DCT2X2", "DCT4X4") else ("DCT4X8/8X4" if name in ("DCT4X8", "DCT8X4") else ("AFV" if s in AFV else bkey))
        want_bucket.append(buckets.setdefault(bkey, len(buckets)))
        want_table.append(tables.setdefault(tkey, len(tables)))
    assert want_bucket == [0, 1, 1, 1, 2, 3, 4, 4, 5, 5, 6, 6, 1, 1, 1, 1, 1, 1, 7, 8, 8, 9, 10, 10, 11, 12, 12]
    assert [want_table[V.S[n]] for n in ("IDENTITY", "DCT2X2", "DCT4X4")] == [1, 2, 3]
    for s in range(V.NUM_STRATEGIES):
        valid, lcx, lcy, bucket, table, flags = _strategy(lib, s)
        assert valid == 1
        assert (1 << lcx, 1 << lcy) == (V.COVERED_X[s], V.COVERED_Y[s]), s
        assert (8 << lcy, 8 << lcx) == _dims(V.NAMES[s]), s
        assert bucket == want_bucket[s] and table == want_table[s], s
        assert bool(flags & 1) == (s in V.SPECIAL or s in AFV), s
        assert bool(flags & 2) == (s in AFV), s
    for s in (-1, V.NUM_STRATEGIES, 255, -(1 << 31)):
        assert _strategy(lib, s)[0] == 0


# ---------------------------------------------------------------- cell info
def test_cell_info_round_trip():
    lib = _lib()
    for s in range(V.NUM_STRATEGIES):
        cx, cy = V.COVERED_X[s], V.COVERED_Y[s]
        lcx, lcy = cx.bit_length() - 1, cy.bit_length() - 1
        for iy in range(cy):
            for ix in range(cx):
                info = lib.jxlhip_selftest_varblock_cell_pack(s, ix, iy, lcx, lcy)
                assert info == (s | ix << 8 | iy << 13 | lcx << 18 | lcy << 21 | 1 << 31)
                assert _unpack(lib, info) == [s, ix, iy, lcx, lcy, 1, int(ix == 0 and iy == 0)]


def test_cell_origin():
    lib = _lib()
    assert _unpack(lib, 0) == [0, 0, 0, 0, 0, 0, 0]
    rng = np.random.default_rng(5)
    words = [0x80000000, 0x00000000, 0x7FFFFFFF, 0xFFFFFFFF, 0x80000100, 0x80002000, 0x8003FF00, 0x80FC00FF, 0x00FC00FF]
    words += [int(w) for w in rng.integers(0, 1 << 32, 200, dtype=np.uint64)]
    words += [int(w) & ~0x3FF00 for w in rng.integers(0, 1 << 32, 200, dtype=np.uint64)]
    for w in words:
        u = _unpack(lib, w)
        assert u[5] == w >> 31
        assert u[6] == int((w >> 31) == 1 and ((w >> 8) & 31) == 0 and ((w >> 13) & 31) == 0), hex(w)
        assert u[6] == int((w & 0x8003FF00) == 0x80000000)


# ---------------------------------------------------------------- stored layout
PLAIN = [s for s in range(V.NUM_STRATEGIES) if s not in V.SPECIAL and s not in AFV]


@pytest.mark.parametrize("s,special", [(s, 0) for s in PLAIN] + [(V.S["DCT4X8"], 1)])
def test_stored_layout(s, special):
    lib = _lib()
    cx, cy = V.COVERED_X[s], V.COVERED_Y[s]
    lcx, lcy = cx.bit_length() - 1, cy.bit_length() - 1
    R, Cc = 8 * cy, 8 * cx
    n = R * Cc
    meta = (C.c_uint32 * 2)()
    index = np.zeros(n, np.uint32)
    back = np.zeros(n, np.uint32)
    llf = np.zeros(n, np.uint8)
    lib.jxlhip_selftest_varblock_stored(C.c_int32(special), C.c_uint32(lcx), C.c_uint32(lcy), meta, index.ctypes.data_as(C.POINTER(C.c_uint32)),
                                        back.ctypes.data_as(C.POINTER(C.c_uint32)), llf.ctypes.data_as(C.POINTER(C.c_uint8)))
    pitch = 8 * max(cx, cy)
    transposed = (not special) and cy >= cx
    assert (1 << meta[0], bool(meta[1])) == (pitch, transposed)
    ky, kx = np.divmod(np.arange(n, dtype=np.int64), Cc)
    want = kx * pitch + ky if transposed else ky * pitch + kx
    assert np.array_equal(index, want)
    assert np.array_equal(np.sort(index), np.arange(64 * cx * cy))   # a bijection onto [0, 64 cx cy)
    assert np.array_equal(back, (ky << 16 | kx).astype(np.uint32))
    assert np.array_equal(llf.astype(bool), (ky < cy) & (kx < cx)) and int(llf.sum()) == cx * cy


def test_basis_offsets_and_team_order():
    lib = _lib()
    off = 0
    for n in (8, 16, 32, 64, 128, 256):   # N x N bases back to back
        assert lib.jxlhip_selftest_varblock_basis_offset(0, n) == off
        off += n * n
    off = 0
    for c in (1, 2, 4, 8, 16, 32):
        assert lib.jxlhip_selftest_varblock_basis_offset(1, c) == off
        off += c * c
    assert [lib.jxlhip_selftest_varblock_channel_of_team(i) for i in range(3)] == [1, 0, 2]   # Y, X, B


# ---------------------------------------------------------------- dequantisation bias
def test_dequant_bias():
    lib = _lib()
    values = [0, 1, -1, 2, -2, 3, -3, 127, -127, 32767, -32767]
    f32 = np.float32
    for qb in (0.93, 0.145, 0.5, 1.0 / 3.0):
        for qb3 in (0.145, 0.93, 0.25, 0.1):
            qb_, qb3_ = f32(qb), f32(qb3)
            for v in values:
                if v == 0:
                    want = want_r = f32(0)
                elif abs(v) == 1:
                    want = want_r = qb_ if v > 0 else -qb_
                else:
                    want = f32(v) - qb3_ / f32(v)
                    want_r = f32(v) - f32(qb3_ * f32(f32(1) / f32(v)))
                got = f32(lib.jxlhip_selftest_varblock_dequant_bias(v, float(qb_), float(qb3_), 0))
                assert got.tobytes() == f32(want).tobytes(), (v, qb, qb3)
                got_r = f32(lib.jxlhip_selftest_varblock_dequant_bias(v, float(qb_), float(qb3_), 1))
                assert got_r.tobytes() == f32(want_r).tobytes(), (v, qb, qb3)


# ---------------------------------------------------------------- LDS layout of recon_tile_kernel
def test_recon_tile_lds():
    lib = _lib()
    out = (C.c_int64 * 14)()
    assert lib.jxlhip_selftest_varblock_recon_lds(out) == 14
    names = ["cfc3", "B816", "cscale", "ci", "cmeta", "cnq", "cpre", "cstart", "ctot", "csc", "t32_lo", "t32_hi", "t64", "end"]
    o = dict(zip(names, out))
    sizes = [3 * 64 * 65 * 4, 320 * 4, 64 * 4, 64 * 4, 64 * 4, 64 * 4, 3 * 64 * 4, 3 * 64 * 4, 4 * 4, 64 * 8, 128 * 16, 128 * 16, 4 * 256 * 16]
    at = 0
    for name, size in zip(names, sizes):   # in the order listed, nothing between them
        assert o[name] == at, name
        at += size
    assert o["end"] == at == 74768 == (3 * 64 * 65 + 320 + 256 + 384 + 4 + 128 + 1024 + 4096) * 4
    assert o["csc"] % 8 == 0
    assert all(o[k] % 16 == 0 for k in ("t32_lo", "t32_hi", "t64"))
