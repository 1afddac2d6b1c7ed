"""CPU tests of jxlhip_save_pixels (include/jxlfiletypeio.h, Part 3): the refusals, which are decided on the host before any device
work, the headers the writer emits for every sample depth and colour encoding, and the struct's layout."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pdn_jpegxl_amd import api
from save_pixels_util import GRAY_PROFILES, save_pixels_raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8, U16, F16, F32 = 0, 1, 2, 3


def desc(buf, w=4, h=3, nch=3, sample_type=U8, bits=8, colour="Srgb", stride=None):
    item = (1, 2, 2, 4)[sample_type] if 0 <= sample_type < 4 else 1
    return api.JxlHipPixels(buf.ctypes.data if buf is not None else None, w, h, w * nch * item if stride is None else stride, nch,
                            sample_type, bits, api.KNOWN_PROFILE.index(colour) if isinstance(colour, str) else colour)


def test_struct_size_is_the_headers():
    hdr = open(os.path.join(ROOT, "include", "jxlfiletypeio.h")).read()
    size = int(re.search(r"static_assert\(sizeof\(JxlHipPixels\) == (\d+)", hdr).group(1))
    assert C.sizeof(api.JxlHipPixels) == size
    assert "jxlhip_save_pixels" in api.EXPORTS and hasattr(api.lib(), "jxlhip_save_pixels")


REFUSALS = [
    ("no size", dict(w=0), "EncodeError", "no pixels"),
    ("no height", dict(h=0), "EncodeError", "no pixels"),
    ("small stride", dict(stride=11), "EncodeError", "stride_bytes"),
    ("small stride u16", dict(sample_type=U16, bits=16, stride=23), "EncodeError", "stride_bytes"),
    ("no channels", dict(nch=0), "EncodeError", "number of channels"),
    ("five channels", dict(nch=5), "EncodeError", "number of channels"),
    ("u8 with 10 bits", dict(bits=10), "EncodeError", "8 for Uint8"),
    ("u16 with 8 bits", dict(sample_type=U16, bits=8), "EncodeError", "9..16"),
    ("u16 with 17 bits", dict(sample_type=U16, bits=17), "EncodeError", "9..16"),
    ("f16 with bits", dict(sample_type=F16, bits=16), "EncodeError", "0 for float"),
    ("f32 with bits", dict(sample_type=F32, bits=32), "EncodeError", "0 for float"),
    ("unknown type", dict(sample_type=4, bits=8), "EncodeError", "sample type"),
    ("gray profile, RGB", dict(colour="LinearGray"), "EncodeError", "gray colour profile"),
    ("gray profile, RGBA", dict(nch=4, colour="GraySrgbTRC"), "EncodeError", "gray colour profile"),
    ("RGB profile, gray", dict(nch=1, colour="DisplayP3"), "EncodeError", "RGB colour profile"),
    ("RGB profile, gray + alpha", dict(nch=2, colour="Rec2020PQ"), "EncodeError", "RGB colour profile"),
    ("BT.709, gray", dict(nch=1, colour="Rec709"), "EncodeError", "RGB colour profile"),
    ("unknown profile", dict(colour=8), "EncodeError", "colour profile"),
    ("null data", dict(null=True), "NullParameter", ""),
]


@pytest.mark.parametrize("kw,status,message", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refusals_are_decided_on_the_host(kw, status, message):
    kw = dict(kw)
    buf = None if kw.pop("null", False) else np.zeros(4096, np.uint8)
    st, msg, writes = save_pixels_raw(desc(buf, **kw))
    assert st == status and message in msg and writes == 0, (st, msg, writes)


def test_refusals_that_depend_on_the_options_and_the_metadata():
    buf = np.zeros(4096, np.uint8)
    for sample_type in (F16, F32):
        st, msg, writes = save_pixels_raw(desc(buf, sample_type=sample_type, bits=0), opt=api.EncoderOptions(1.0, 7, True))
        assert st == "EncodeError" and "lossless float" in msg and writes == 0
    icc = np.zeros(128, np.uint8)
    md = api.EncoderImageMetadata(None, 0, icc.ctypes.data, len(icc), None, 0)
    st, msg, writes = save_pixels_raw(desc(buf), md=md)
    assert st == "EncodeError" and "ICC" in msg and writes == 0
    L = api.lib()
    err = api.ErrorInfo()
    d, opt, md, io = desc(buf), api.EncoderOptions(1.0, 7, False), api.EncoderImageMetadata(), api.IOCallbacks()
    null = api.ENCODER_STATUS.index("NullParameter")
    assert L.jxlhip_save_pixels(None, C.byref(opt), C.byref(md), C.byref(io), C.byref(err), api.ProgressFn()) == null
    assert L.jxlhip_save_pixels(C.byref(d), None, C.byref(md), C.byref(io), C.byref(err), api.ProgressFn()) == null
    assert L.jxlhip_save_pixels(C.byref(d), C.byref(opt), None, C.byref(io), C.byref(err), api.ProgressFn()) == null
    assert L.jxlhip_save_pixels(C.byref(d), C.byref(opt), C.byref(md), None, C.byref(err), api.ProgressFn()) == null
    assert save_pixels_raw(d, with_write=False)[0] == "NullParameter"   # a callbacks struct without Write
    # the two profiles that stand for their gray counterparts are NOT refused with 1 or 2 channels: the first refusal such a call can
    # meet is a later one (here: lossless floats), so it got past the colour check without touching the device
    for colour in ("Srgb", "LinearSrgb"):
        st, msg, _ = save_pixels_raw(desc(buf, nch=2, sample_type=F32, bits=0, colour=colour), opt=api.EncoderOptions(1.0, 7, True))
        assert st == "EncodeError" and "lossless float" in msg


def _headers(w, h, gray, alpha, lossless, bits, exp_bits, colour):
    L = api.selftest_lib()
    L.jxlhip_selftest_headers_deep.restype = C.c_size_t
    L.jxlhip_selftest_headers_deep.argtypes = [C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_int32,
                                               C.c_void_p, C.c_size_t]
    buf = (C.c_uint8 * (1 << 16))()
    n = L.jxlhip_selftest_headers_deep(w, h, gray, alpha, lossless, bits, exp_bits, api.KNOWN_PROFILE.index(colour), buf, len(buf))
    assert n > 0
    return bytes(buf[:n])


DEPTHS = [(8, 0), (9, 0), (10, 0), (12, 0), (13, 0), (16, 0), (16, 5), (32, 8)]


@pytest.mark.parametrize("lossless", [0, 1], ids=["lossy", "lossless"])
@pytest.mark.parametrize("bits,exp_bits", DEPTHS, ids=["u8", "u9", "u10", "u12", "u13", "u16", "f16", "f32"])
def test_headers_parse_back_to_what_was_stated(bits, exp_bits, lossless):
    for colour in api.KNOWN_PROFILE:
        gray = colour in GRAY_PROFILES
        for g in ([1] if gray else ([0, 1] if colour in ("Srgb", "LinearSrgb") else [0])):
            for alpha in (0, 1):
                data = _headers(300, 200, g, alpha, lossless, bits, exp_bits, colour)
                info = api.peek(data)
                assert (info.width, info.height) == (300, 200)
                assert info.num_channels == (1 if g else 3) + alpha and info.has_alpha == alpha
                assert info.bytes_per_sample == (4 if exp_bits == 8 else (2 if bits > 8 else 1)), (bits, exp_bits, colour)
                assert info.reserved == (1 if exp_bits else 0)
                assert api.parse_check(data)[0] in ("Ok", "DecodeError")   # the headers parse; the (empty) sections need not


def test_eight_bit_srgb_headers_are_the_bytes_they_were():
    L = api.selftest_lib()
    L.jxlhip_selftest_headers.restype = C.c_size_t
    L.jxlhip_selftest_headers.argtypes = [C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]
    for w, h in ((300, 200), (64, 64), (2100, 300)):
        for gray in (0, 1):
            for alpha in (0, 1):
                for lossless in (0, 1):
                    buf = (C.c_uint8 * (1 << 16))()
                    n = L.jxlhip_selftest_headers(w, h, gray, alpha, lossless, 1, 3, buf, len(buf))
                    assert n > 0
                    want = bytes(buf[:n])
                    assert _headers(w, h, gray, alpha, lossless, 8, 0, "GraySrgbTRC" if gray else "Srgb") == want
    # and those bytes are what the writer emitted before it knew other depths: container, signature, size, "8-bit integers, one
    # default alpha channel, XYB, enumerated sRGB / D65 / perceptual" for a 64 x 64 RGBA lossy frame
    data = _headers(64, 64, 0, 1, 0, 8, 0, "Srgb")
    cs = data[data.index(b"jxlc") + 4:]
    assert cs[:2] == b"\xff\x0a"
    bits = "".join(format(b, "08b")[::-1] for b in cs[2:12])   # LSB first
    size = "1" + "11100" + "100"                                # small, 64 / 8 - 1 = 7, ratio 1 (every field LSB first)
    meta = "0" + "0" + "0" + "00" + "1" + "10" + "1" + "1"      # not default, no extra fields, int, 8 bits, 16-bit buffers, one extra channel: default alpha, XYB
    colour = "0" + "0" + "00" + "10" + "10" + "0" + "01" + "1101" + "00"   # not default, no ICC, RGB, D65, sRGB primaries, no gamma, tf 13 = 2 + 11, perceptual
    assert bits.startswith(size + meta + colour + "00" + "1"), bits
