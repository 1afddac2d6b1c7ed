"""CPU tests of animation encode: the image and frame headers the writer emits for the frames of an animation, read
back with the tests' own reader (layer_util), and the rules that turn change extents into frame rectangles (csrc/enc_animation.cc)
against a short model.  Both go through the test library's hooks; no GPU."""
import ctypes as C
import itertools
import os
import re

import pytest

import animation_util as AU
import encode_animation_util as EU
import layer_util as LU
from pdn_jpegxl_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANVAS = (300000, 200000)   # large enough for every range of the crop code


def headers(xsize=CANVAS[0], ysize=CANVAS[1], gray=0, alpha=0, lossless=0, anim=None, crop=None, duration=0, is_last=1, save=0, source=0,
            bits=8, exp_bits=0, epf=1):
    """The bare codestream of jxlhip_selftest_animation_headers: image header, one frame header, the TOC's first bit.  anim: (tps
    numerator, tps denominator, loops) or None; crop: (x0, y0, w, h) or None."""
    L = api.selftest_lib()
    fn = L.jxlhip_selftest_animation_headers
    fn.restype = C.c_size_t
    fn.argtypes = [C.POINTER(C.c_int64), C.c_void_p, C.c_size_t]
    a = anim or (0, 0, 0)
    c = crop or (0, 0, 0, 0)
    v = [xsize, ysize, gray, alpha, lossless, 1 if anim else 0, a[0], a[1], a[2], 1 if crop else 0, c[0], c[1], c[2], c[3], duration, is_last,
         save, source, bits, exp_bits, epf]
    buf = (C.c_uint8 * 4096)()
    n = fn((C.c_int64 * len(v))(*v), buf, len(buf))
    assert n > 0
    return bytes(buf[:n])


def animation_fields(cs):
    """(tps numerator, tps denominator, loops, have_timecodes), read like animation_util.with_animation_header reads them."""
    r = LU.BitReader(cs, 16)
    small = r.b()
    dim = (lambda: r.u(5)) if small else (lambda: r.u32(LU.B(9, 1), LU.B(13, 1), LU.B(18, 1), LU.B(30, 1)))
    dim()
    if r.u(3) == 0:
        dim()
    assert not r.b() and r.b()           # not all_default, extra fields
    assert r.u(3) == 0                   # orientation 1
    assert not r.b() and not r.b()       # no intrinsic size, no preview
    assert r.b()                         # have_animation
    return r.u32(*AU.TPS_NUM), r.u32(*AU.TPS_DEN), r.u32(*AU.LOOPS), r.b()


TPS_NUMERATORS = [100, 1000, 777, (1 << 29) + 12345, 1, 1024, 1025, 1 << 30]     # the four code ranges and their ends
TPS_DENOMINATORS = [1, 1001, 200, 1000, 256, 257, 1024]
LOOPS = [0, 5, 7, 8, 40000, 65535, 65536, (1 << 32) - 1]


@pytest.mark.parametrize("lossless", [0, 1], ids=["lossy", "lossless"])
@pytest.mark.parametrize("alpha", [0, 1], ids=["opaque", "alpha"])
def test_animation_header_fields_come_back(alpha, lossless):
    n = max(len(TPS_NUMERATORS), len(TPS_DENOMINATORS), len(LOOPS))
    for k in range(n):
        want = (TPS_NUMERATORS[k % len(TPS_NUMERATORS)], TPS_DENOMINATORS[k % len(TPS_DENOMINATORS)], LOOPS[k % len(LOOPS)])
        cs = headers(640, 480, alpha=alpha, lossless=lossless, anim=want, duration=3, is_last=0, save=1)
        assert animation_fields(cs) == want + (False,), want
        info = LU.read_image_header(cs)
        assert (info.xsize, info.ysize, info.nec, info.xyb) == (640, 480, alpha, not lossless)
        assert info.have_animation and not info.have_timecodes
        h, _ = LU.read_frame_header(cs, info.frame_start, info, (640, 480))
        assert h.duration == 3 and not h.is_last and h.save_ref == 1 and h.crop is None


# offsets and sizes in each range of the crop code (8, 11, 14 and 30 bits; offsets are coded as 2 * x0), with the ends of the ranges
CROP_OFFSETS = [0, 1, 100, 127, 128, 1000, 1151, 1152, 5000, 9343, 9344, 20000, 250000]
CROP_SIZES = [1, 255, 256, 2303, 2304, 18687, 18688, 40000]
DURATIONS = [1, 255, 256, (1 << 32) - 1, 2, 257]


@pytest.mark.parametrize("lossless", [0, 1], ids=["lossy", "lossless"])
@pytest.mark.parametrize("alpha", [0, 1], ids=["opaque", "alpha"])
def test_frame_header_fields_come_back(alpha, lossless):
    W, H = CANVAS
    crops = [None, (0, 0, W, H), (0, 0, 1, 1)]
    for k, x0 in enumerate(CROP_OFFSETS):
        y0 = CROP_OFFSETS[(k + 5) % len(CROP_OFFSETS)]
        cw, ch = CROP_SIZES[k % len(CROP_SIZES)], CROP_SIZES[(k + 3) % len(CROP_SIZES)]
        if y0 + ch > H:
            y0 = H - ch
        crops.append((x0, y0, cw, ch))
    for k, crop in enumerate(crops):
        for position in ("first", "middle", "last"):
            duration = DURATIONS[(k + len(position)) % len(DURATIONS)]
            is_last = position == "last"
            cs = headers(alpha=alpha, lossless=lossless, anim=(100, 1, 0), crop=crop, duration=duration, is_last=int(is_last),
                         save=0 if is_last else 1, source=1)
            info = LU.read_image_header(cs)
            assert info.have_animation and info.nec == alpha
            h, end = LU.read_frame_header(cs, info.frame_start, info, CANVAS)
            assert h.frame_type == 0 and h.encoding == lossless
            assert h.crop == crop, (crop, h.crop)
            partial = crop is not None and crop != (0, 0, W, H)
            assert len(h.blending) == 1 + alpha
            for bl in h.blending:
                assert bl.mode == 0 and bl.source == (1 if partial else 0)
            assert h.duration == duration and h.is_last == is_last
            assert h.save_ref == (0 if is_last else 1) and h.save_before_ct is False and h.name == b""
            # the reader stopped where the writer did: one TOC bit, then the padding to a byte
            assert not LU.BitReader(cs, end).b() and (end + 1 + 7) // 8 == len(cs)


def test_default_fields_write_the_bytes_of_a_still():
    """With the animation and placement fields at their defaults the writers emit what they emitted before they had them: the
    single-frame headers of the existing hook, a frame header spelled out by hand, and the reader's view of a still."""
    L = api.selftest_lib()
    L.jxlhip_selftest_headers.restype = C.c_size_t
    L.jxlhip_selftest_headers.argtypes = [C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]
    for (w, h), gray, alpha, lossless, epf in itertools.product(((300, 200), (64, 64), (2100, 300)), (0, 1), (0, 1), (0, 1), (0, 1, 2, 3)):
        buf = (C.c_uint8 * (1 << 16))()
        n = L.jxlhip_selftest_headers(w, h, gray, alpha, lossless, epf, 3, buf, len(buf))
        still = bytes(buf[:n])
        still = still[still.index(b"jxlc") + 4:]
        mine = headers(w, h, gray=gray, alpha=alpha, lossless=lossless, epf=epf)
        assert still[:len(mine)] == mine
        info = LU.read_image_header(mine)
        assert not info.have_animation
        fh, end = LU.read_frame_header(mine, info.frame_start, info, (w, h))
        assert fh.crop is None and fh.is_last and fh.duration == 0 and fh.save_ref == 0 and all(b.mode == 0 and b.source == 0 for b in fh.blending)
        assert (end + 1 + 7) // 8 == len(mine)
    # a lossless gray 64 x 64 frame, field by field (every field LSB first): not all_default, regular frame, Modular, no flags, no
    # YCbCr, no upsampling, group size shift 1, one pass, no crop, replace, is_last, no name, loop filter (not default: no Gaborish,
    # no EPF, no extensions), no extensions, then the TOC's "not permuted"
    mine = headers(64, 64, gray=1, lossless=1)
    info = LU.read_image_header(mine)
    bits = "".join(format(b, "08b")[::-1] for b in mine[info.frame_start:])
    want = "0" + "00" + "1" + "00" + "0" + "00" + "10" + "00" + "0" + "00" + "1" + "00" + "0" + "0" + "00" + "00" + "00" + "0"
    assert bits.startswith(want) and set(bits[len(want):]) <= {"0"} and len(bits) == (len(want) + 7) // 8 * 8


def test_struct_and_exports():
    hdr = open(os.path.join(ROOT, "include", "jxlfiletypeio.h")).read()
    size = int(re.search(r"static_assert\(sizeof\(JxlHipAnimationOptions\) == (\d+)", hdr).group(1))
    assert C.sizeof(api.AnimationOptions) == size
    for name in ("jxlhip_encode_animation", "jxlhip_encoder_animation_rects"):
        assert name in api.EXPORTS and hasattr(api.lib(), name)


# ---------------------------------------------------------------- the rectangle rules
def rects(extents, durations, w, h, lossless, key_interval):
    L = api.selftest_lib()
    fn = L.jxlhip_selftest_animation_rects
    fn.restype = None
    fn.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    n = len(extents) + 1
    flat = [v for e in extents for v in (e if e is not None else (-1, -1, -1, -1))]
    out = (C.c_int32 * (9 * n))()
    fn(n, (C.c_int32 * max(len(flat), 1))(*flat), (C.c_uint32 * n)(*durations), w, h, lossless, key_interval, out)
    return [tuple(out[9 * k:9 * k + 9]) for k in range(n)]


def model(extents, durations, w, h, lossless, key_interval):
    """The rules of the issue, frame by frame: (x, y, width, height, have_crop, duration, is_last, save slot, source slot)."""
    n = len(extents) + 1
    out = []
    for k in range(n):
        r = EU.model_rect(k, extents[k - 1] if k else None, w, h, lossless, key_interval)
        last = k == n - 1
        out.append(r + (int(r != (0, 0, w, h)), durations[k], int(last), 0 if last else 1, 1))
    return out


@pytest.mark.parametrize("lossless", [0, 1], ids=["lossy", "lossless"])
@pytest.mark.parametrize("key_interval", [0, 1, 3])
def test_rectangles_follow_the_rules(key_interval, lossless):
    for w, h in itertools.product((1, 7, 8, 9, 257), repeat=2):
        px = lambda x, y: (x, y, x, y)
        extents = [None, px(0, 0), px(w - 1, 0), px(0, h - 1), px(w - 1, h - 1), px(w // 2, h // 2), (0, 0, w - 1, h - 1), None,
                   (w // 3, h // 4, w - 1 - w // 5, h - 1 - h // 7), (0, h // 2, w - 1, h // 2), (w // 2, 0, w // 2, h - 1)]
        durations = [1 + 37 * k for k in range(len(extents) + 1)]
        got = rects(extents, durations, w, h, lossless, key_interval)
        assert got == model(extents, durations, w, h, lossless, key_interval), (w, h)
        for k, g in enumerate(got):   # whatever the rules say, a rectangle lies on the canvas and holds what changed
            x, y, rw, rh = g[:4]
            assert 0 <= x and 0 <= y and rw >= 1 and rh >= 1 and x + rw <= w and y + rh <= h
            e = extents[k - 1] if k else None
            if e is not None:
                assert x <= e[0] and y <= e[1] and x + rw > e[2] and y + rh > e[3]
            if not lossless and g[4] and e is not None:   # (an unchanged frame is one pixel, lossy too)
                assert x % 8 == 0 and y % 8 == 0 and ((x + rw) % 8 == 0 or x + rw == w) and ((y + rh) % 8 == 0 or y + rh == h)


def test_a_single_frame_is_the_canvas_and_the_last():
    assert rects([], [5], 33, 17, 0, 0) == [(0, 0, 33, 17, 0, 5, 1, 0, 1)]
