"""Layered JPEG XL codestreams for the tests, built from single-frame files of the oracle.

A layered file is the image header of an oracle encode of the canvas size, followed by the frames of separately encoded layer files,
each with its frame header rewritten (crop, blending, is_last, duration, save_as_reference, name).  The TOC sizes and the sections
are copied verbatim: frames start byte-aligned, and the TOC's bit-packed sizes start at a byte boundary after one `permuted` bit.

The header reader / writer here is written from the frame header's field list on its own (not from the library's writer), so a field
order mistake cannot agree with itself.
"""
from dataclasses import dataclass, field
from typing import List, Optional


class BitReader:
    def __init__(self, data: bytes, pos: int = 0):
        self.data, self.pos = data, pos

    def u(self, n):
        v = 0
        for k in range(n):
            byte = self.data[(self.pos + k) >> 3]
            v |= ((byte >> ((self.pos + k) & 7)) & 1) << k
        self.pos += n
        return v

    def b(self):
        return self.u(1) == 1

    def u32(self, *dists):   # each dist: ("v", value) or ("b", bits, offset)
        d = dists[self.u(2)]
        return d[1] if d[0] == "v" else d[2] + self.u(d[1])

    def u64(self):
        s = self.u(2)
        if s == 0:
            return 0
        if s == 1:
            return 1 + self.u(4)
        if s == 2:
            return 17 + self.u(8)
        v, shift = self.u(12), 12
        while self.u(1):
            if shift == 60:
                v |= self.u(4) << 60
                break
            v |= self.u(8) << shift
            shift += 8
        return v

    def f16(self):
        return self.u(16)

    def enum(self):
        return self.u32(("v", 0), ("v", 1), ("b", 4, 2), ("b", 6, 18))


class BitWriter:
    def __init__(self):
        self.bits: List[int] = []

    def u(self, n, v):
        assert 0 <= v < (1 << n) or n == 0, (n, v)
        self.bits += [(v >> k) & 1 for k in range(n)]

    def b(self, v):
        self.u(1, 1 if v else 0)

    def u32(self, v, *dists):
        for sel, d in enumerate(dists):
            if d[0] == "v" and v == d[1]:
                return self.u(2, sel)
        for sel, d in enumerate(dists):
            if d[0] == "b" and d[2] <= v < d[2] + (1 << d[1]):
                self.u(2, sel)
                return self.u(d[1], v - d[2])
        raise ValueError("value %d not representable" % v)

    def raw(self, bits):
        self.bits += list(bits)

    def align(self):
        while len(self.bits) % 8:
            self.bits.append(0)

    def tobytes(self):
        assert len(self.bits) % 8 == 0
        out = bytearray(len(self.bits) // 8)
        for i, bit in enumerate(self.bits):
            out[i >> 3] |= bit << (i & 7)
        return bytes(out)


def _bits_of(data, start, end):
    return [(data[i >> 3] >> (i & 7)) & 1 for i in range(start, end)]


V = lambda v: ("v", v)
B = lambda n, o=0: ("b", n, o)
CROP = (B(8), B(11, 256), B(14, 2304), B(30, 18688))
NAME_LEN = (V(0), B(4), B(5, 16), B(10, 48))


@dataclass
class ImageInfo:
    xsize: int
    ysize: int
    nec: int
    xyb: bool
    have_animation: bool
    have_timecodes: bool
    frame_start: int   # byte offset of the first frame header in the codestream


def read_image_header(cs: bytes) -> ImageInfo:
    """The image header of a bare codestream (no container, no embedded ICC profile), up to the first frame."""
    assert cs[:2] == b"\xff\x0a", "bare codestream expected"
    r = BitReader(cs, 16)

    def size():
        small = r.b()
        dim = (lambda: (r.u(5) + 1) * 8) if small else (lambda: r.u32(B(9, 1), B(13, 1), B(18, 1), B(30, 1)))
        ys = dim()
        ratio = r.u(3)
        num, den = [0, 1, 12, 4, 3, 16, 5, 2], [0, 1, 10, 3, 2, 9, 4, 1]
        xs = ys * num[ratio] // den[ratio] if ratio else dim()
        return xs, ys

    def bit_depth():
        if not r.b():
            r.u32(V(8), V(10), V(12), B(6, 1))
        else:
            r.u32(V(32), V(16), V(24), B(6, 1))
            r.u(4)

    xs, ys = size()
    nec, xyb, anim, tc, extra = 0, True, False, False, False
    if not r.b():
        extra = r.b()
        if extra:
            r.u(3)
            if r.b():
                size()
            assert not r.b(), "preview"
            anim = r.b()
            if anim:
                r.u32(V(100), V(1000), B(10, 1), B(30, 1))
                r.u32(V(1), V(1001), B(8, 1), B(10, 1))
                r.u32(V(0), B(3), B(16), B(32))
                tc = r.b()
        bit_depth()
        r.b()
        nec = r.u32(V(0), V(1), B(4, 2), B(12, 1))
        for _ in range(nec):
            if r.b():
                continue
            t = r.enum()
            bit_depth()
            r.u32(V(0), V(3), V(4), B(3, 1))
            nl = r.u32(V(0), B(4), B(5, 16), B(10, 48))
            r.u(8 * nl)
            if t == 0:
                r.b()
            if t == 2:
                r.u(64)
            if t == 5:
                r.u32(V(1), B(2), B(4, 3), B(8, 19))
        xyb = r.b()
        if not r.b():   # colour encoding
            want_icc = r.b()
            assert not want_icc, "embedded ICC profiles are not handled here"
            cspace = r.enum()
            xy = lambda: r.u32(B(19), B(19, 524288), B(20, 1048576), B(21, 2097152))
            if cspace != 2:
                wp = r.enum()
                if wp == 2:
                    xy(), xy()
            if cspace not in (1, 2):
                pr = r.enum()
                if pr == 2:
                    for _ in range(6):
                        xy()
            if cspace != 2:
                if r.b():
                    r.u(24)
                else:
                    r.enum()
            r.enum()
        if extra and not r.b():
            r.f16(), r.f16(), r.b(), r.f16()
        ext = r.u64()
        total = sum(r.u64() for i in range(64) if ext >> i & 1)
        r.pos += total
    if not r.b():   # custom transform data
        if xyb and not r.b():
            r.pos += 16 * 16
        mask = r.u(3)
        r.pos += (16 * 15 if mask & 1 else 0) + (16 * 55 if mask & 2 else 0) + (16 * 210 if mask & 4 else 0)
    pos = (r.pos + 7) // 8
    return ImageInfo(xs, ys, nec, xyb, anim, tc, pos)


@dataclass
class Blending:
    mode: int = 0
    alpha: int = 0
    clamp: bool = False
    source: int = 0


@dataclass
class FrameHeader:
    prefix: list                       # bits from frame_type up to (not including) have_crop, verbatim
    ups_at: int = -1                   # position in prefix of the colour upsampling selector (-1: absent)
    frame_type: int = 0
    encoding: int = 0
    crop: Optional[tuple] = None       # (x0, y0, w, h)
    blending: List[Blending] = field(default_factory=list)
    duration: int = 0
    timecode: int = 0
    is_last: bool = True
    save_ref: int = 0
    save_before_ct: bool = False
    name: bytes = b""
    tail: list = field(default_factory=list)   # loop filter + extensions, verbatim


def _pack(v):
    return 2 * v if v >= 0 else -2 * v - 1


def _unpack(u):
    return (u >> 1) ^ -(u & 1)


def read_frame_header(cs: bytes, pos_bytes: int, info: ImageInfo, canvas):
    """Returns (FrameHeader, bit position right after it).  canvas = (w, h) of the image the frame belongs to."""
    r = BitReader(cs, pos_bytes * 8)
    assert not r.b(), "all-default frame headers are not handled here"
    start = r.pos
    ftype, enc = r.u(2), r.u(1)
    flags = r.u64()
    ycbcr = (not info.xyb) and r.b()
    lf = bool(flags & 32)
    if ycbcr and not lf:
        r.u(6)
    ups_at = -1
    if not lf:
        ups_at = r.pos - start
        r.u32(V(1), V(2), V(4), V(8))
        for _ in range(info.nec):
            r.u32(V(1), V(2), V(4), V(8))
    if enc == 1:
        r.u(2)
    if enc == 0 and info.xyb:
        r.u(3), r.u(3)
    if ftype != 2:
        passes = r.u32(V(1), V(2), V(3), B(3, 4))
        if passes != 1:
            nds = r.u32(V(0), V(1), V(2), B(1, 3))
            r.u(2 * (passes - 1))
            for _ in range(nds):
                r.u32(V(1), V(2), V(4), V(8))
            for _ in range(nds):
                r.u32(V(0), V(1), V(2), B(3))
    if ftype == 1:
        r.u32(V(1), V(2), V(3), V(4))
    h = FrameHeader(prefix=_bits_of(cs, start, r.pos), ups_at=ups_at, frame_type=ftype, encoding=enc)
    if ftype != 1 and r.b():
        x0 = y0 = 0
        if ftype != 2:
            x0, y0 = _unpack(r.u32(*CROP)), _unpack(r.u32(*CROP))
        h.crop = (x0, y0, r.u32(*CROP), r.u32(*CROP))
    full = _full(h.crop, canvas)
    normal = ftype in (0, 3)
    if normal:
        for _ in range(1 + info.nec):
            bl = Blending(mode=r.u32(V(0), V(1), V(2), B(2, 3)))
            if info.nec and bl.mode in (2, 3):
                bl.alpha = r.u32(V(0), V(1), V(2), B(3, 3))
            if info.nec and 2 <= bl.mode <= 4:
                bl.clamp = r.b()
            if bl.mode != 0 or not full:
                bl.source = r.u(2)
            h.blending.append(bl)
        if info.have_animation:
            h.duration = r.u32(V(0), V(1), B(8), B(32))
            if info.have_timecodes:
                h.timecode = r.u(32)
        h.is_last = r.b()
    else:
        h.is_last = False
    if ftype != 1 and not h.is_last:
        h.save_ref = r.u(2)
    if ftype != 1:
        can_ref = not h.is_last and (h.duration == 0 or h.save_ref != 0)
        if ftype == 2 or (full and h.blending[0].mode == 0 and can_ref):
            h.save_before_ct = r.b()
    nl = r.u32(*NAME_LEN)
    h.name = bytes(r.u(8) for _ in range(nl))
    tail_start = r.pos
    # loop filter
    if not r.b():
        gab = r.b()
        if gab and r.b():
            r.u(16 * 6)
        epf = r.u(2)
        if epf:
            if enc == 0 and r.b():
                r.u(16 * 8)
            if r.b():
                r.u(16 * 3), r.u(32)
            if r.b():
                if enc == 0:
                    r.u(16)
                r.u(16 * 3)
            if enc == 1:
                r.u(16)
        assert r.u64() == 0
    ext = r.u64()
    r.pos += sum(r.u64() for i in range(64) if ext >> i & 1)
    h.tail = _bits_of(cs, tail_start, r.pos)
    return h, r.pos


def _full(crop, canvas):
    if crop is None:
        return True
    x0, y0, w, h = crop
    return x0 <= 0 and y0 <= 0 and x0 + w >= canvas[0] and y0 + h >= canvas[1]


def write_frame_header(h: FrameHeader, info: ImageInfo, canvas) -> list:
    w = BitWriter()
    w.b(False)
    w.u(2, h.frame_type)
    w.raw(h.prefix[2:])
    if h.frame_type != 1:
        w.b(h.crop is not None)
        if h.crop is not None:
            x0, y0, cw, ch = h.crop
            if h.frame_type != 2:
                w.u32(_pack(x0), *CROP)
                w.u32(_pack(y0), *CROP)
            w.u32(cw, *CROP)
            w.u32(ch, *CROP)
    full = _full(h.crop, canvas)
    if h.frame_type in (0, 3):
        assert len(h.blending) == 1 + info.nec
        for bl in h.blending:
            w.u32(bl.mode, V(0), V(1), V(2), B(2, 3))
            if info.nec and bl.mode in (2, 3):
                w.u32(bl.alpha, V(0), V(1), V(2), B(3, 3))
            if info.nec and 2 <= bl.mode <= 4:
                w.b(bl.clamp)
            if bl.mode != 0 or not full:
                w.u(2, bl.source)
        if info.have_animation:
            w.u32(h.duration, V(0), V(1), B(8), B(32))
            if info.have_timecodes:
                w.u(32, h.timecode)
        w.b(h.is_last)
    if h.frame_type != 1 and not h.is_last:
        w.u(2, h.save_ref)
    if h.frame_type != 1:
        can_ref = not h.is_last and (h.duration == 0 or h.save_ref != 0)
        if h.frame_type == 2 or (full and h.blending[0].mode == 0 and can_ref):
            w.b(h.save_before_ct)
    w.u32(len(h.name), *NAME_LEN)
    for c in h.name:
        w.u(8, c)
    w.raw(h.tail)
    return w.bits


@dataclass
class Layer:
    """One frame of a layered file: a bare single-frame codestream of the oracle and how it is placed and blended."""
    cs: bytes
    x0: int = 0
    y0: int = 0
    crop: bool = True          # False: no crop (the layer file must then be of the canvas size)
    blending: Optional[List[Blending]] = None   # [colour, extra channel 0, ...]; None: replace everything
    duration: int = 0
    save_ref: int = 0
    name: bytes = b""
    frame_type: Optional[int] = None   # override (refusal tests only)
    upsampling2: bool = False          # mark the frame as upsampled x2 (refusal tests only)
    flags: int = 0                     # frame flags (refusal tests only: 2 patches, 32 LF frame)
    save_before_ct: bool = False


def frame_of(cs: bytes):
    """(ImageInfo, FrameHeader, bit position after the header) of a single-frame bare codestream."""
    info = read_image_header(cs)
    h, end = read_frame_header(cs, info.frame_start, info, (info.xsize, info.ysize))
    return info, h, end


def reemit_frame(cs: bytes, h: FrameHeader, info: ImageInfo, canvas, end_bits: int) -> bytes:
    """The frame with header h in place of its own: header, `permuted` = 0, then the TOC sizes and the sections verbatim."""
    r = BitReader(cs, end_bits)
    assert not r.b(), "permuted TOCs are not handled here"
    toc = (r.pos + 7) // 8
    w = BitWriter()
    w.raw(write_frame_header(h, info, canvas))
    w.b(False)
    w.align()
    return w.tobytes() + cs[toc:]


def layered(canvas_cs: bytes, layers: List[Layer], last_is_last=True) -> bytes:
    """canvas_cs: an oracle encode (bare codestream) of the canvas size with the image header all layers share (bit depth, channels,
    animation).  The last layer gets is_last (unless last_is_last is False)."""
    cinfo = read_image_header(canvas_cs)
    canvas = (cinfo.xsize, cinfo.ysize)
    out = canvas_cs[:cinfo.frame_start]
    for k, L in enumerate(layers):
        info, h, end = frame_of(L.cs)
        info = ImageInfo(info.xsize, info.ysize, cinfo.nec, cinfo.xyb, cinfo.have_animation, cinfo.have_timecodes, info.frame_start)
        assert info.nec == read_image_header(L.cs).nec
        if L.crop:
            h.crop = (L.x0, L.y0, info.xsize, info.ysize)
        else:
            assert (info.xsize, info.ysize) == canvas
            h.crop = None
        if L.frame_type == 2 and h.frame_type != 2:   # a reference-only frame has no num_passes field (a single pass: selector 0)
            assert h.prefix[-2:] == [0, 0]
            h.prefix = h.prefix[:-2]
        if L.frame_type is not None:
            h.frame_type = L.frame_type
        if L.upsampling2:
            h.prefix = h.prefix[:h.ups_at] + [1, 0] + h.prefix[h.ups_at + 2:]
        if L.flags:
            # flags follow frame_type (2 bits) and encoding (1): the layer's own are 0 (U64 selector 0); an LF frame has no upsampling fields
            assert h.prefix[3:5] == [0, 0]
            if L.flags & 32:
                h.prefix = h.prefix[:h.ups_at] + h.prefix[h.ups_at + 2 + 2 * cinfo.nec:]
            w = BitWriter()
            if L.flags <= 16:
                w.u(2, 1), w.u(4, L.flags - 1)
            else:
                w.u(2, 2), w.u(8, L.flags - 17)
            h.prefix = h.prefix[:3] + w.bits + h.prefix[5:]
        h.blending = [Blending(b.mode, b.alpha, b.clamp, b.source) for b in (L.blending or [Blending() for _ in range(1 + cinfo.nec)])]
        h.duration = L.duration
        h.is_last = last_is_last and k == len(layers) - 1
        h.save_ref = L.save_ref
        h.save_before_ct = L.save_before_ct
        h.name = L.name
        out += reemit_frame(L.cs, h, info, canvas, end)
    return out
