"""CPU tests of a decode batch's memory layout (csrc/batch_layout.h, no GPU), through one export of the test library that parses and plans
files, lays their batch out measuring and then placing - the blob in a host buffer, fake bases for everything else - and reports the
allocation logs, what the placed DevImages point at and a read-back of the blob.  What must hold of a layout - the two passes agree,
allocations neither overlap nor leave their region, no two fields share memory except where the design says so, the sizes of a few
buffers from the frame's geometry - is written out here on its own, not taken from the code under test."""
import ctypes as C

import numpy as np
import pytest

import icc_util
import noise_util
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth
from test_entropy_plan import check_pieces, streams as plan_streams   # noqa: F401  (the fixture)

BLOB, ZERO, WS, OUT, STATIC, PIX = range(6)
HEAD = ["n", "n_extra", "pixel_chunk", "m_blob", "m_zero", "m_ws", "p_blob", "p_zero", "p_ws", "cmp", "bad", "threw", "guard_ok", "m_pix", "p_pix"]
REC = ["image", "status", "decoded", "all_zero", "encoding", "w", "h", "w8", "h8", "ng", "nlf", "cs_size", "cs_region", "cs_off", "cmp", "bad"]
# the pointers of a DevImage that the export lists, in its order
FIELDS = ["lf0", "lf1", "lf2", "lf_tmp0", "lf_tmp1", "lf_tmp2", "lf_final0", "lf_final1", "lf_final2", "lfq0", "lfq1", "lfq2", "lf_extra", "cellinfo",
          "rawq", "sharp", "ytox", "ytob", "binfo", "lf_desc", "lf_count", "alpha_desc", "blk_list", "blk_count", "grp_bitpos", "alpha_bitpos", "lf_end_bits",
          "mod_plane0", "mod_plane1", "mod_plane2", "mod_plane3", "mod_plane4", "mod_desc", "wp_lf", "wp_grp", "lz_lf", "lz_grp", "lz_hf", "lz_mod", "alpha32",
          "centries", "cblk", "coef0", "coef1", "coef2", "tmp0", "tmp1", "tmp2", "xyb0", "xyb1", "xyb2", "xyb2_0", "xyb2_1", "xyb2_2", "inv_sigma", "tile_list",
          "alpha", "out", "status", "noise_rnd0", "noise_rnd1", "noise_rnd2", "noise0", "noise1", "noise2", "ds_alpha", "ds_out"]
CHUNK = ["tmp0", "tmp1", "tmp2", "xyb0", "xyb1", "xyb2", "coef0", "coef1", "coef2", "noise0", "noise1", "noise2"]   # planes shared by images a chunk apart
# a field that is, by design, another field's memory
ALIAS = {"xyb2_0": "coef0", "xyb2_1": "coef1", "xyb2_2": "coef2", "noise_rnd0": "tmp0", "noise_rnd1": "tmp1", "noise_rnd2": "tmp2"}
PASS_OWNS = ["centries", "cblk", "grp_bitpos", "lz_hf"]   # what a later pass's record does not share with its frame's

_L = None


def _lib():
    global _L
    if _L is None:
        _L = api.selftest_lib()
        _L.jxlhip_selftest_batch_layout.restype = C.c_size_t
        _L.jxlhip_selftest_batch_layout.argtypes = [C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                                     C.c_size_t]
    return _L


def layout_of(files, band=(0, 0), downscale=1, debug_taps=False):
    n = len(files)
    data = (C.c_char_p * n)(*files)
    sizes = (C.c_size_t * n)(*[len(f) for f in files])
    opts = (C.c_int32 * 7)(band[0], band[1], downscale, 0, 0, 0, int(debug_taps))
    cap = 1 << 16
    while True:
        buf = np.zeros(cap, np.int64)
        k = _lib().jxlhip_selftest_batch_layout(n, data, sizes, opts, buf.ctypes.data_as(C.POINTER(C.c_int64)), cap)
        if k:
            break
        cap *= 4
        assert cap <= 1 << 26
    v = buf[:k].tolist()
    pos = [0]

    def take(m):
        pos[0] += m
        return v[pos[0] - m:pos[0]]
    B = dict(zip(HEAD, take(len(HEAD))))
    for name in ("log_m", "log_p"):
        m = take(1)[0]
        flat = take(4 * m)
        B[name] = [tuple(flat[4 * j:4 * j + 4]) for j in range(m)]   # (region, offset, bytes, align)
    B["recs"] = []
    for _ in range(B["n"] + B["n_extra"]):
        r = dict(zip(REC, take(len(REC))))
        m = take(1)[0]
        flat = take(3 * m)
        r["fields"] = {FIELDS[flat[3 * j]]: (flat[3 * j + 1], flat[3 * j + 2]) for j in range(m)}   # name -> (region, offset)
        m = take(1)[0]
        flat = take(4 * m)
        r["cfg"] = [tuple(flat[4 * j:4 * j + 4]) for j in range(m)]   # (split, msb, lsb, packed word)
        B["recs"].append(r)
    assert pos[0] == k
    return B


def check_layout(B, debug_taps=False):
    n = B["n"]
    # 1. the two passes agree: the same allocations, and the placing pass ends exactly where the measuring pass did
    assert B["log_m"] == B["log_p"] and B["log_m"]
    assert (B["p_blob"], B["p_zero"], B["p_ws"], B["p_pix"]) == (B["m_blob"], B["m_zero"], B["m_ws"], B["m_pix"])
    # 2. within a region the allocations lie in order, each at its alignment, without overlap, none past the total
    starts = {}
    for region, total in ((BLOB, B["m_blob"]), (ZERO, B["m_zero"]), (WS, B["m_ws"]), (PIX, B["m_pix"])):
        log = [e for e in B["log_m"] if e[0] == region]
        for e in log:
            assert e[3] >= 1 and e[3] & (e[3] - 1) == 0
        check_pieces([e[1] for e in log], [e[2] for e in log], total, 0, [e[3] for e in log])
        starts[region] = {e[1]: e[2] for e in log if e[2]}   # non-empty allocations by offset (an empty one shares its offset with the next)
    assert {e[0] for e in B["log_m"]} <= {BLOB, ZERO, WS, PIX}
    # 3. read-back of the tables, 6. failed parses
    assert B["bad"] == 0 and B["cmp"] >= 6
    for r in B["recs"]:
        if not r["decoded"]:
            assert r["all_zero"] and not r["fields"]
            continue
        assert not r["all_zero"] and r["bad"] == 0 and r["cmp"] > 0, r
        assert (r["cs_region"], starts[BLOB][r["cs_off"]]) == (BLOB, r["cs_size"] + 16)   # (no file of these is resident on a device)
        assert r["cfg"]
        for split, msb, lsb, word in r["cfg"]:
            assert word & 0xFFF == split | msb << 4 | lsb << 8
            assert word >> 12 == 0 or word >> 12 & 1   # an ordinary cluster is nothing more; a one-symbol cluster has bit 12 and its symbol
    # 4. no aliasing
    used = {}   # (region, offset) -> [(record, field)]
    for k, r in enumerate(B["recs"]):
        f = r["fields"]
        main = B["recs"][r["image"]]["fields"]
        for name, (region, off) in f.items():
            if name in ("out", "ds_out") and region == OUT:
                assert off == r["image"] << 34   # the caller's buffer of this image
                continue
            if name == "status":
                assert (region, off) == (ZERO, 64 * r["image"]) and starts[ZERO][0] == 64 * max(1, n)
                continue
            shared = name in CHUNK or name in ALIAS   # the planes that chunks of frames share have a region of their own
            assert region == (ZERO if name == "cellinfo" else PIX if shared else WS), (name, region)
            assert off in starts[region], (k, name, off)   # it starts an allocation
            if k >= n and name not in PASS_OWNS:
                assert main[name] == (region, off), (k, name)   # a pass's record is a copy of its frame's
                continue
            if name in ALIAS:
                assert f[ALIAS[name]] == (region, off), (k, name)
                continue
            if name.startswith("lf_final"):
                assert (region, off) in (f["lf" + name[-1]], f["lf_tmp" + name[-1]])
                continue
            if name == "alpha_bitpos":   # the end positions of the frame's last pass
                last = [q for q in B["recs"] if q["image"] == r["image"]][-1]
                assert last["fields"]["grp_bitpos"] == (region, off)
                continue
            used.setdefault((region, off), []).append((k, name))
    for (region, off), users in used.items():
        if len(users) == 1:
            continue
        # only the chunk planes are shared: by the same field of images a whole number of chunks apart
        names = {name for _, name in users}
        assert len(names) == 1 and names <= set(CHUNK) and not debug_taps, users
        assert len({k % B["pixel_chunk"] for k, _ in users}) == 1 and all(k < n for k, _ in users), users
    if n > B["pixel_chunk"]:   # ... and they are
        vardct = [k for k in range(n) if B["recs"][k]["decoded"] and B["recs"][k]["encoding"] == 0 and "tmp0" in B["recs"][k]["fields"]]
        for k in vardct:
            for j in vardct:
                if j > k and (j - k) % B["pixel_chunk"] == 0:
                    for name in CHUNK[:9]:
                        assert B["recs"][k]["fields"][name] == B["recs"][j]["fields"][name]
    # 7. a region that is placing refuses what it did not measure, and writes nothing
    assert B["threw"] == 1 and B["guard_ok"] == 1
    return starts


@pytest.fixture(scope="module")
def streams(oracle, plan_streams):   # noqa: F811
    def img(w, h, seed, nch=4):
        return np.ascontiguousarray(synth(w, h, seed)[..., :nch])
    S = dict(plan_streams)
    S["200x150 orientation 6"] = oracle.encode(img(200, 150, 21, 3), orientation=6)
    S["300x280 orientation 3, lossless"] = oracle.encode(img(300, 280, 22), lossless=True, lossless_tree=1, lossless_predictor=5, orientation=3)
    S["300x280 custom orders"] = oracle.encode(img(300, 280, 23, 3), custom_orders=True)
    S["300x280 custom quant tables"] = oracle.encode(img(300, 280, 24), custom_quant_tables=True)
    S["513x300 2 passes, custom orders"] = oracle.encode(img(513, 300, 25, 3), num_passes=2, custom_orders=True)
    S["90x70 noise"] = noise_util.noisy(oracle.encode(img(90, 70, 27), container=False), list(range(0, 512, 64)))
    S["200x150 icc tone curves"] = oracle.encode(img(200, 150, 26, 3), icc=icc_util.matrix_profile())
    return S


THREE_ROWS = ["64x600 rgba", "300x600 2 passes"]
VARIANTS = [dict(), dict(band=(1, 1)), dict(downscale=8), dict(debug_taps=True)]


@pytest.mark.parametrize("opts", VARIANTS, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()) or "defaults")
def test_layout_of_single_images_and_of_a_mixed_batch(streams, opts):
    names = THREE_ROWS if "band" in opts else list(streams)
    batches = [[k] for k in names] + [names]
    for batch in batches:
        B = layout_of([streams[k] for k in batch], **opts)
        assert all(r["decoded"] for r in B["recs"]), batch
        check_layout(B, debug_taps=opts.get("debug_taps", False))
        assert B["pixel_chunk"] == (len(batch) if opts.get("debug_taps") else min(len(batch), 32))
        if opts.get("downscale") == 8:   # no reconstruction, no filters: no pixel planes
            assert not any(name in r["fields"] for r in B["recs"] for name in CHUNK)


def test_more_images_than_a_pixel_chunk_share_planes(streams):
    files = [streams[k] for k in ("8x8 rgba", "200x150 rgb", "64x64 lossless gradient", "257x257 rgba", "513x300 2 passes")] * 14
    B = layout_of(files)
    assert B["n"] == 70 and B["pixel_chunk"] == 32
    check_layout(B)
    a, b = B["recs"][0]["fields"], B["recs"][64]["fields"]
    assert a["tmp0"] == b["tmp0"] and a["xyb1"] == b["xyb1"] and a["coef2"] == b["coef2"] and a["lf0"] != b["lf0"]
    B = layout_of(files[:40], debug_taps=True)
    assert B["pixel_chunk"] == 40
    check_layout(B, debug_taps=True)


def test_streams_reach_the_branches_they_are_meant_to(streams, oracle):
    B = layout_of(list(streams.values()))
    by = dict(zip(streams, B["recs"]))
    assert by["200x150 orientation 6"]["fields"]["out"][0] == WS and by["300x280 orientation 3, lossless"]["fields"]["out"][0] == WS
    assert by["200x150 rgb"]["fields"]["out"][0] == OUT
    assert by["90x70 noise"]["fields"]["noise0"][0] == PIX and "noise0" not in by["200x150 rgb"]["fields"]
    assert "lz_hf" in by["300x280 lz77"]["fields"] and "lz_mod" in by["300x280 lossless prefix+lz77"]["fields"]
    assert "wp_grp" in by["300x300 lossless weighted"]["fields"] and "mod_plane2" in by["300x300 lossless weighted"]["fields"]
    assert B["n_extra"] == 1 + 2 + 1 + 1
    # frames with their own coefficient orders or dequantisation tables have tables in the blob that the same image without them has not
    tables = lambda files: sum(1 for e in layout_of(files)["log_m"] if e[0] == BLOB and e[2])   # noqa: E731
    for k, seed, nch in (("300x280 custom orders", 23, 3), ("300x280 custom quant tables", 24, 4)):
        assert tables([streams[k]]) > tables([oracle.encode(np.ascontiguousarray(synth(300, 280, seed)[..., :nch]))])
    icc = layout_of([streams["200x150 icc tone curves"]])
    assert any(e[0] == BLOB and e[2] == 4 * 3 * 4096 for e in icc["log_m"])
    assert not any(e[0] == BLOB and e[2] == 4 * 3 * 4096 for e in layout_of([streams["200x150 rgb"]])["log_m"])


def test_sizes_from_the_geometry(streams):
    B = layout_of([streams["257x257 rgba"]])
    starts = check_layout(B)
    r = B["recs"][0]
    w, h = 257, 257
    w8, h8 = (w + 7) // 8, (h + 7) // 8
    ng, nlf = ((w + 255) // 256) * ((h + 255) // 256), ((w + 2047) // 2048) * ((h + 2047) // 2048)
    assert (r["w"], r["h"], r["w8"], r["h8"], r["ng"], r["nlf"]) == (w, h, w8, h8, ng, nlf)
    size = lambda name: starts[r["fields"][name][0]][r["fields"][name][1]]   # noqa: E731
    for c in "012":
        assert size("lfq" + c) == 4 * w8 * h8
    assert size("rawq") == 2 * w8 * h8
    assert size("blk_list") == ng * 4096
    assert size("alpha32") == 4 * w * h
    assert starts[BLOB][r["cs_off"]] == r["cs_size"] + 16


def test_failed_parses_leave_zeroed_records(streams):
    good = streams["257x257 rgba"]
    B = layout_of([good, good[:len(good) // 8], b"\xff\x0a" + bytes(30), streams["300x300 lossless gradient"]])
    assert [r["decoded"] for r in B["recs"]] == [1, 0, 0, 1]
    check_layout(B)
    for r in B["recs"][1:3]:
        assert r["all_zero"] and not r["fields"] and r["cs_region"] == -1
