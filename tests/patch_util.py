"""Patched JPEG XL files for the tests: reference-only (type 2) atlas frames and frames that carry a patch dictionary.

A patched frame is an oracle encode whose section 0 (LfGlobal, or the only section of a one-group frame) gets the dictionary's bits in
front of it; the TOC entry of that section is rewritten (sections have no internal byte alignment).  layer_util then sets the patches
flag in the frame header and places the frames.  The dictionary stream is written by the library's own entropy-code writer through the
test library (jxlhip_selftest_write_tokens); its field order is written here from the format description.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import layer_util as LU

# contexts of the dictionary stream
NUM_REF, REF_FRAME, SIZE, REF_POS, POS, MODE, OFFSET, COUNT, ALPHA, CLAMP = range(10)
# patch blend modes
NONE, REPLACE, ADD, MUL, BLEND_ABOVE, BLEND_BELOW, AWADD_ABOVE, AWADD_BELOW = range(8)


@dataclass
class Place:
    """One position of a reference patch: (x, y) in the patched frame, and one (mode, alpha_channel, clamp) record per channel group
    (colour, then each extra channel)."""
    x: int
    y: int
    blend: List[Tuple[int, int, bool]] = field(default_factory=lambda: [(REPLACE, 0, False)])


@dataclass
class Ref:
    """A rectangle (x0, y0, w, h) of the reference frame in `slot` and the positions it is blended at."""
    slot: int
    x0: int
    y0: int
    w: int
    h: int
    places: List[Place] = field(default_factory=list)


def pack_signed(v):
    return 2 * v if v >= 0 else -2 * v - 1


def tokens(refs: List[Ref], nec: int, raw_deltas: Optional[dict] = None):
    """The (context, value) stream of a dictionary.  Positions after a reference's first are coded as deltas from the previous one;
    raw_deltas {(ref index, place index): (dx_token, dy_token)} overrides the coded delta tokens (out-of-range tests)."""
    out = [(NUM_REF, len(refs))]
    for i, r in enumerate(refs):
        out += [(REF_FRAME, r.slot), (REF_POS, r.x0), (REF_POS, r.y0), (SIZE, r.w - 1), (SIZE, r.h - 1), (COUNT, len(r.places) - 1)]
        prev = None
        for j, p in enumerate(r.places):
            if prev is None:
                out += [(POS, p.x), (POS, p.y)]
            elif raw_deltas and (i, j) in raw_deltas:
                out += [(OFFSET, raw_deltas[(i, j)][0]), (OFFSET, raw_deltas[(i, j)][1])]
            else:
                out += [(OFFSET, pack_signed(p.x - prev.x)), (OFFSET, pack_signed(p.y - prev.y))]
            prev = p
            assert len(p.blend) == 1 + nec, (len(p.blend), nec)
            for mode, alpha, clamp in p.blend:
                out.append((MODE, mode))
                if 4 <= mode <= 7 and nec > 1:
                    out.append((ALPHA, alpha))
                if 3 <= mode <= 7:
                    out.append((CLAMP, int(clamp)))
    return out


def write_tokens(toks, num_ctx=10):
    """(bytes, bit count) of the entropy-coded stream (code header + tokens)."""
    from pdn_jpegxl_amd import api
    L = api.selftest_lib()
    f = L.jxlhip_selftest_write_tokens
    f.restype = C.c_size_t
    f.argtypes = [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64)]
    n = len(toks)
    ctxs = (C.c_uint32 * max(1, n))(*[c for c, _ in toks])
    vals = (C.c_uint32 * max(1, n))(*[v for _, v in toks])
    cap = 64 + 8 * n + 4096
    buf = C.create_string_buffer(cap)
    nbits = C.c_uint64(0)
    size = f(num_ctx, ctxs, vals, n, buf, cap, C.byref(nbits))
    assert size > 0, "token writer failed"
    return buf.raw[:size], nbits.value


def _bits(data: bytes, nbits: int):
    return [(data[i >> 3] >> (i & 7)) & 1 for i in range(nbits)]


def _num_sections(cs: bytes, info, h):
    """TOC entries of a single-frame oracle encode (its geometry: no crop, one pass)."""
    assert h.encoding == 1, "patched frames are Modular"
    at = h.ups_at + 2 + 2 * info.nec   # group_size_shift follows the upsampling selectors (all 1: selector 0)
    assert h.prefix[h.ups_at:at] == [0] * (at - h.ups_at)
    gdim = 128 << (h.prefix[at] | h.prefix[at + 1] << 1)
    cdiv = lambda a, b: (a + b - 1) // b
    ng = cdiv(info.xsize, gdim) * cdiv(info.ysize, gdim)
    nlf = cdiv(info.xsize, 8 * gdim) * cdiv(info.ysize, 8 * gdim)
    return 1 if ng == 1 else 2 + nlf + ng


TOC = (LU.B(10), LU.B(14, 1024), LU.B(22, 17408), LU.B(30, 4211712))


def with_dictionary(cs: bytes, dict_bytes: bytes, dict_bits: int) -> bytes:
    """The single-frame bare codestream cs with dict_bits bits of dict_bytes in front of its section 0 (TOC rewritten)."""
    info, h, end = LU.frame_of(cs)
    r = LU.BitReader(cs, end)
    assert not r.b(), "permuted TOCs are not handled here"
    r.pos = (r.pos + 7) // 8 * 8
    n = _num_sections(cs, info, h)
    sizes = [r.u32(*TOC) for _ in range(n)]
    data = (r.pos + 7) // 8
    assert data + sum(sizes) == len(cs), (data, sizes, len(cs))
    sec0 = LU.BitWriter()
    sec0.raw(_bits(dict_bytes, dict_bits))
    sec0.raw(_bits(cs[data:data + sizes[0]], 8 * sizes[0]))
    sec0.align()
    s0 = sec0.tobytes()
    w = LU.BitWriter()
    w.raw(LU._bits_of(cs, info.frame_start * 8, end))
    w.b(False)
    w.align()
    for s in [len(s0)] + sizes[1:]:
        w.u32(s, *TOC)
    w.align()
    return cs[:info.frame_start] + w.tobytes() + s0 + cs[data + sizes[0]:]


def patched(cs: bytes, refs: List[Ref], nec: int, raw_deltas=None, extra_tokens=()) -> bytes:
    """cs with the dictionary of `refs` (extra_tokens: appended after it, for stream-damage tests)."""
    data, nbits = write_tokens(tokens(refs, nec, raw_deltas) + list(extra_tokens))
    return with_dictionary(cs, data, nbits)
