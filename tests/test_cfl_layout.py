"""CPU checks of what fitted chroma-from-luma maps add to the encoder's buffers (csrc/enc_batch_layout.h), through the test library's
layout hook (test_encode_batch_layout.py): an image without them lays out what it always did; with them it gets the two maps and room
for their tokens in front of the block-info rows of every LF group."""
import ctypes as C

from pdn_jpegxl_amd import api


def up(v):
    return (max(v, 256) + 255) // 256 * 256


def layout(items):
    """items: (w, h, channels, bytes per sample, lossless, fitted maps).  The hook's totals, and per image (measured, placed) of every
    buffer it has (csrc/selftest.cc: jxlhip_selftest_enc_batch_layout)."""
    f = api.selftest_lib().jxlhip_selftest_enc_batch_layout
    f.restype = C.c_size_t
    f.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_size_t]
    flat = (C.c_int32 * (6 * len(items)))(*[v for it in items for v in it])
    n = f(len(items), flat, None, 0)
    out = (C.c_int64 * n)()
    assert f(len(items), flat, out, n) == n
    v = list(out)
    d = {"measured": v[1], "placed": v[2], "images": []}
    at = 19
    for _ in range(v[0]):
        count = v[at + 5]
        d["images"].append([(v[at + 6 + 3 * k + 1], v[at + 6 + 3 * k + 2]) for k in range(count)])
        at += 6 + 3 * count
    assert at == len(v)
    return d


def test_fitting_adds_the_maps_and_the_room_for_their_tokens():
    w, h = 3840, 2160
    off, on = layout([(w, h, 4, 1, 0, 0)]), layout([(w, h, 4, 1, 0, 1)])
    assert on["measured"] == on["placed"] and off["measured"] == off["placed"]
    ntile = ((w + 63) // 64) * ((h + 63) // 64)
    nlf = ((w + 2047) // 2048) * ((h + 2047) // 2048)
    nsec = nlf + ((w + 255) // 256) * ((h + 255) // 256) + 1
    k_lf, k_meta, k_cfl, k_ac, k_alpha, per_tok = 3 * 65536, 2 * 65536, 2 * 1024, 3 * 65 * 1024, 65536, 6
    cap = lambda meta: (max(k_lf + meta, k_ac + k_alpha) * per_tok + 256) & ~15
    want = 2 * up(ntile) + up(nlf * (k_meta + k_cfl) * 8) - up(nlf * k_meta * 8) + up(nsec * cap(k_meta + k_cfl)) - up(nsec * cap(k_meta))
    assert on["placed"] - off["placed"] == want


def test_a_lossless_image_ignores_the_option():
    assert layout([(300, 280, 4, 1, 1, 1)])["placed"] == layout([(300, 280, 4, 1, 1, 0)])["placed"]


def test_mixed_batch_places_what_it_measures():
    d = layout([(65, 130, 3, 1, 0, 1), (300, 280, 4, 2, 0, 0), (2112, 72, 3, 1, 0, 1), (9, 9, 2, 2, 1, 1)])
    assert d["measured"] == d["placed"] > 0
    for im in d["images"]:
        assert im and all(measured == placed for measured, placed in im)
