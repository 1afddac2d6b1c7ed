"""CPU checks of the batch encoder's workspace layout (csrc/enc_batch_layout.cc: LayEncBatch) through the test library: the measuring
pass and the placing pass agree, nothing overlaps, every counter lies in the head that one memset clears, and the bytes of a 4K image
are what DESIGN.md §4.6 states - recomputed here from the capacities of csrc/enc_types.h."""
import ctypes as C
import os
import re

import pytest

from pdn_jpegxl_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the order of `fields` in jxlhip_selftest_enc_batch_layout
FIELDS = (["xyb%d" % c for c in range(3)] + ["pad%d" % c for c in range(3)] + ["alpha_px"] + ["lfq%d" % c for c in range(3)]
          + ["rawq", "act", "strat"] + ["qs%d" % c for c in range(3)] + ["nz%d" % c for c in range(3)] + ["nzc%d" % c for c in range(3)]
          + ["last%d" % c for c in range(3)] + ["tok_lf", "tok_meta", "tok_ac", "tok_alpha", "n_ac", "n_meta", "hist_mod", "hist_ac"]
          + ["ll_plane%d" % c for c in range(4)] + ["tok_ll", "sec_bytes", "stream_state", "sec_bits"])
HEAD = {"hist_mod": 0, "hist_ac": 0, "sec_bits": 1, "n_ac": 2, "n_meta": 2, "stream_state": 2}   # field -> region of the head


def layout(items):
    """items: (w, h, channels, bytes per sample, lossless).  Returns the hook's answer as a dict."""
    f = api.selftest_lib().jxlhip_selftest_enc_batch_layout
    f.restype = C.c_size_t
    f.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_size_t]
    flat = (C.c_int32 * (6 * len(items)))(*[v for w, h, c, b, ll in items for v in (w, h, c, b, ll, 0)])
    n = f(len(items), flat, None, 0)
    out = (C.c_int64 * n)()
    assert f(len(items), flat, out, n) == n
    v = list(out)
    names = ["n", "measured", "placed", "head_bytes", "r0", "r1", "r2", "r3", "tables", "records_m", "mcodes", "records_a", "acodes", "dst_off",
             "body", "total_sections", "sizeof_image", "mod_code_bytes", "hf_code_bytes"]
    d = dict(zip(names, v))
    at = len(names)
    d["images"] = []
    for _ in range(d["n"]):
        begin, end, src, surface, sections, count = v[at:at + 6]
        at += 6
        fields = {}
        for k in range(count):
            fid, measured, placed = v[at + 3 * k:at + 3 * k + 3]
            fields[FIELDS[fid]] = (measured, placed)
        at += 3 * count
        d["images"].append({"begin": begin, "end": end, "src": src, "surface": surface, "sections": sections, "fields": fields})
    assert at == len(v)
    return d


MIXED = [(1, 1, 1, 1, 0), (264, 200, 4, 2, 0), (256, 256, 4, 1, 1), (2056, 16, 3, 1, 0), (9, 9, 2, 2, 1), (264, 200, 3, 4, 0), (3840, 2160, 4, 1, 0)]


def test_measuring_and_placing_agree():
    d = layout(MIXED)
    assert d["measured"] == d["placed"] > 0
    for im in d["images"]:
        assert im["fields"]
        for name, (measured, placed) in im["fields"].items():
            assert measured == placed, name


def test_regions_are_ordered_and_buffers_do_not_overlap():
    d = layout(MIXED)
    bounds = [d[k] for k in ("r0", "r1", "r2", "r3", "tables", "records_m", "mcodes", "records_a", "acodes", "dst_off", "body")]
    assert bounds[0] == 0 and bounds == sorted(bounds) and d["r3"] == d["head_bytes"] and all(b % 256 == 0 for b in bounds)
    assert d["mcodes"] - d["records_m"] >= d["n"] * d["sizeof_image"] and d["acodes"] - d["records_a"] >= d["n"] * d["sizeof_image"]
    assert d["records_a"] - d["mcodes"] >= d["n"] * d["mod_code_bytes"]
    lossy = sum(1 for it in MIXED if not it[4])
    assert d["dst_off"] - d["acodes"] >= lossy * d["hf_code_bytes"]
    assert d["body"] - d["dst_off"] >= 8 * (d["total_sections"] + 1)
    assert d["total_sections"] == sum(im["sections"] for im in d["images"])
    regions = [(d["r0"], d["r1"]), (d["r1"], d["r2"]), (d["r2"], d["r3"])]
    offsets = []
    prev_end = d["body"]
    for it, im in zip(MIXED, d["images"]):
        assert prev_end <= im["begin"] <= im["src"] and im["end"] <= d["placed"] and im["begin"] % 256 == 0
        prev_end = im["end"]
        body = [im["src"]] + ([im["surface"]] if it[3] == 1 else [])
        assert (im["surface"] == im["src"]) == (it[3] != 1)
        for name, (_, off) in im["fields"].items():
            assert off % 256 == 0, name
            if name in HEAD:
                lo, hi = regions[HEAD[name]]
                assert lo <= off < hi, name
            else:
                assert im["begin"] <= off < im["end"], name
                body.append(off)
            offsets.append(off)
        assert len(set(body)) == len(body)
        # which buffers an image has follows from what it is
        lossless, alpha = bool(it[4]), it[2] in (2, 4)
        assert ("tok_ll" in im["fields"]) == lossless and ("tok_ac" in im["fields"]) == (not lossless) and ("hist_ac" in im["fields"]) == (not lossless)
        assert ("tok_alpha" in im["fields"]) == (alpha and not lossless)
    assert len(set(offsets)) == len(offsets)


def test_a_batch_of_equal_images_grows_by_the_same_bytes_per_image():
    one, two, five = (layout([(300, 280, 4, 1, 0)] * k)["placed"] for k in (1, 2, 5))
    assert (five - two) == 3 * (two - one)


def up(v):
    return (max(v, 256) + 255) // 256 * 256


def test_bytes_of_a_4k_image_are_what_design_md_states():
    """3840 x 2160 RGBA8, lossy: every buffer from the capacities of csrc/enc_types.h, each rounded up to 256 bytes."""
    w, h = 3840, 2160
    npx, w8, h8 = w * h, (w + 7) // 8, (h + 7) // 8
    ncell, npad = w8 * h8, w8 * 8 * h8 * 8
    ng, nlf = ((w + 255) // 256) * ((h + 255) // 256), ((w + 2047) // 2048) * ((h + 2047) // 2048)
    k_lf, k_meta, k_ac, k_alpha, syms, ac_ctx, leaves, per_tok = 3 * 65536, 2 * 65536, 3 * 65 * 1024, 65536, 128, 495 * 15, 9, 6
    nsec = nlf + ng + 1
    sec_cap = (max(k_lf + k_meta, k_ac + k_alpha) * per_tok + 256) & ~15
    body = [npx * 4, npx * 4]                                          # the caller's pixels in tight rows, the BGRA8 surface
    body += [npx * 4] * 3 + [npad * 4] * 3 + [ncell * 4] * 3 + [ncell * 256] * 3 + [ncell] * 3 + [ncell * 2] * 6   # xyb, pad, lfq, qs, nz, nzc, last
    body += [ncell * 4, ncell * 4, ncell, npx * 4]                     # rawq, act, strat, alpha_px
    body += [nlf * k_lf * 8, nlf * k_meta * 8, ng * k_ac * 8, ng * k_alpha * 8, nsec * sec_cap]
    head = [leaves * syms * 4, ac_ctx * syms * 4], [nsec * 8], [ng * 4, nlf * 4, (2 * (nlf + ng) + 1) * 4]
    d = layout([(w, h, 4, 1, 0)])
    small = d["body"] - d["head_bytes"]                                # tables, records, room for the codes, compaction offsets
    want = sum(sum(up(b) for b in region) for region in head) + small + sum(up(b) for b in body)
    assert d["placed"] == want
    assert small < 1 << 20
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"([\d,]+) bytes per 3840 x 2160 RGBA8 image", text)
    assert m, "DESIGN.md states the bytes per image"
    assert int(m.group(1).replace(",", "")) == d["placed"]


@pytest.mark.parametrize("item", [(3840, 2160, 4, 1, 1), (3840, 2160, 4, 2, 0)], ids=["lossless", "rgba16"])
def test_other_kinds_of_image_take_less_or_more_as_their_buffers_say(item):
    base = layout([(3840, 2160, 4, 1, 0)])["placed"]
    got = layout([item])["placed"]
    if item[4]:
        assert got < base          # four integer planes and one token array instead of the lossy planes, tokens and sections
    else:
        assert got == base         # 16-bit input: twice the pixels, no BGRA8 surface
