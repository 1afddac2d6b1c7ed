"""Helpers of the animation tests: the decode plan through the test library, animation headers with other field values, frames with
timecodes, and the model of the rules that the plan is checked against.

The model is written from the frame list the test built (test_gpu_layers.F), not from what the parser read: which frames complete a
displayed image, which are saved, which slots a frame reads, and which slots are alive where a chunk ends.
"""
import ctypes as C

import numpy as np

import layer_util as LU
from pdn_jpegxl_amd import api

MAX_CHUNK_FRAMES = 64   # kMaxLayerFrames: frames of one launch


class Plan:
    pass


def plan(data, chunk_frames=0, counts=(0,), scratch_budget=0):
    """jxlhip_selftest_animation_plan as an object: header fields, `frames` (dicts) and `chunks` (dicts).  Raises api.FormatError with
    the parser's message where the file is refused."""
    L = api.selftest_lib()
    fn = L.jxlhip_selftest_animation_plan
    fn.restype = C.c_size_t
    fn.argtypes = [C.c_char_p, C.c_size_t, C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int64), C.c_size_t, C.POINTER(C.c_int32),
                   C.POINTER(api.ErrorInfo)]
    cap = 1 << 16
    out = (C.c_int64 * cap)()
    cnt = (C.c_int32 * len(counts))(*counts)
    st, err = C.c_int32(0), api.ErrorInfo()
    n = fn(data, len(data), chunk_frames, scratch_budget, cnt, len(counts), out, cap, C.byref(st), C.byref(err))
    if n == 0:
        raise api.FormatError(api.DECODER_STATUS[st.value], err.errorMessage.decode("ascii", "replace"))
    v = list(out[:n])
    p = Plan()
    (nfr, p.num_displayed, p.have_animation, p.tps_numerator, p.tps_denominator, p.num_loops, p.have_timecodes, p.raw, p.width,
     p.height, p.single) = v[:11]
    at = 11
    p.frames = []
    keys = ["show", "duration", "timecode", "save", "reads", "source", "mode", "asource", "amode", "partial", "scratch", "live_after"]
    for _ in range(nfr):
        fr = dict(zip(keys, v[at:at + len(keys)]))
        nl = v[at + len(keys)]
        at += len(keys) + 1
        fr["name"] = bytes(v[at:at + nl])
        at += nl
        p.frames.append(fr)
    nchunks = v[at]
    at += 1
    ck = ["call", "first", "count", "first_shown", "shown", "live_in", "live_out"]
    p.chunks = [dict(zip(ck, v[at + 7 * i:at + 7 * i + 7])) for i in range(nchunks)]
    assert at + 7 * nchunks == n
    return p


# ---------------------------------------------------------------- files
TPS_NUM = (LU.V(100), LU.V(1000), LU.B(10, 1), LU.B(30, 1))
TPS_DEN = (LU.V(1), LU.V(1001), LU.B(8, 1), LU.B(10, 1))
LOOPS = (LU.V(0), LU.B(3), LU.B(16), LU.B(32))


def with_animation_header(canvas_cs, tps_numerator, tps_denominator, num_loops, have_timecodes):
    """The bare canvas codestream (an oracle encode with an animation header) with other values in the header's four fields.  Only the
    image header is kept right: the result is what LU.layered / frames_with_timecodes take as their canvas."""
    info = LU.read_image_header(canvas_cs)
    assert info.have_animation
    # the true end of the image header (read_image_header returns it rounded up to a byte): walk it again with a reader we can see
    seen = []

    class Spy(LU.BitReader):
        def __init__(self, *a):
            super().__init__(*a)
            seen.append(self)

    orig, LU.BitReader = LU.BitReader, Spy
    try:
        LU.read_image_header(canvas_cs)
    finally:
        LU.BitReader = orig
    end = seen[0].pos
    r = LU.BitReader(canvas_cs, 16)
    small = r.b()
    dim = (lambda: r.u(5)) if small else (lambda: r.u32(LU.B(9, 1), LU.B(13, 1), LU.B(18, 1), LU.B(30, 1)))
    dim()
    if r.u(3) == 0:
        dim()
    assert not r.b() and r.b()           # not all_default, extra fields
    r.u(3)                               # orientation
    assert not r.b() and not r.b()       # no intrinsic size, no preview
    assert r.b()                         # have_animation
    start = r.pos
    r.u32(*TPS_NUM), r.u32(*TPS_DEN), r.u32(*LOOPS), r.b()
    w = LU.BitWriter()
    w.raw(LU._bits_of(canvas_cs, 0, start))
    w.u32(tps_numerator, *TPS_NUM)
    w.u32(tps_denominator, *TPS_DEN)
    w.u32(num_loops, *LOOPS)
    w.b(have_timecodes)
    w.raw(LU._bits_of(canvas_cs, r.pos, end))
    w.align()
    return w.tobytes()


def frames_with_timecodes(canvas_cs, layers, timecodes):
    """LU.layered for plain layers (placement, blending, duration, save slot, name), with a timecode per frame."""
    cinfo = LU.read_image_header(canvas_cs)
    canvas = (cinfo.xsize, cinfo.ysize)
    out = canvas_cs[:cinfo.frame_start]
    for k, (L, tc) in enumerate(zip(layers, timecodes)):
        info, h, end = LU.frame_of(L.cs)
        info = LU.ImageInfo(info.xsize, info.ysize, cinfo.nec, cinfo.xyb, cinfo.have_animation, cinfo.have_timecodes, info.frame_start)
        h.crop = (L.x0, L.y0, info.xsize, info.ysize) if L.crop else None
        h.blending = [LU.Blending(b.mode, b.alpha, b.clamp, b.source) for b in (L.blending or [LU.Blending() for _ in range(1 + cinfo.nec)])]
        h.duration, h.timecode, h.is_last, h.save_ref, h.name = L.duration, tc, k == len(layers) - 1, L.save_ref, L.name
        out += LU.reemit_frame(L.cs, h, info, canvas, end)
    return out


# ---------------------------------------------------------------- the model
def shows(frames):
    """Per frame: the displayed image it completes (-1: none).  frames: test_gpu_layers.F, the last one is is_last."""
    out, j = [], 0
    for k, fr in enumerate(frames):
        shown = k == len(frames) - 1 or fr.duration > 0
        out.append(j if shown else -1)
        j += shown
    return out


def saves(frames):
    """Per frame: the slot it is saved to (-1: not saved): not the last frame, and no duration or a slot other than 0."""
    return [fr.save if k != len(frames) - 1 and (fr.duration == 0 or fr.save != 0) else -1 for k, fr in enumerate(frames)]


def reads(fr, W, H):
    """The slots frame fr reads: the source of a channel group that blends, or that shows outside a crop smaller than the canvas."""
    fh, fw = fr.px.shape[:2]
    x0, y0 = (fr.x0, fr.y0) if fr.crop else (0, 0)
    partial = not (x0 <= 0 and y0 <= 0 and x0 + fw >= W and y0 + fh >= H)
    s = set()
    if fr.mode != 0 or partial:
        s.add(fr.source)
    if fr.amode != 0 or partial:
        s.add(fr.asource)
    return s


def live_behind(frames, W, H, e):
    """Mask of the slots alive at a cut behind frame e: some frame up to e was saved there, and walking on from e + 1 the slot is read
    before it is saved to again."""
    sv = saves(frames)
    mask = 0
    for s in range(4):
        if s not in sv[:e + 1]:
            continue
        for k in range(e + 1, len(frames)):
            if s in reads(frames[k], W, H):
                mask |= 1 << s
                break
            if sv[k] == s:
                break
    return mask


def model_chunks(frames, W, H, chunk_frames, counts, scratch=None, budget=None):
    """The chunks of successive next(count) calls (count <= 0: everything left): a chunk ends behind the frame that completes the last
    image asked for, after min(chunk_frames or 64, 64) frames, or - scratch: bytes per frame, budget: bytes per chunk - in front of the
    frame that would take the chunk's scratch past the budget; it always holds one frame."""
    sh = shows(frames)
    total = max(sh) + 1
    cap = min(chunk_frames, MAX_CHUNK_FRAMES) if chunk_frames >= 1 else MAX_CHUNK_FRAMES
    out, nf, ns = [], 0, 0
    for call, count in enumerate(counts):
        n = total - ns if count <= 0 else min(count, total - ns)
        last = ns + n - 1
        while ns <= last:
            cnt = 0
            shown = 0
            used = 0
            while nf + cnt < len(frames) and cnt < cap:
                if budget is not None and cnt > 0 and used + scratch[nf + cnt] > budget:
                    break
                if budget is not None:
                    used += scratch[nf + cnt]
                cnt += 1
                if sh[nf + cnt - 1] >= 0:
                    shown += 1
                    if sh[nf + cnt - 1] >= last:
                        break
            out.append(dict(call=call, first=nf, count=cnt, shown=shown, live_in=live_behind(frames, W, H, nf - 1) if nf else 0,
                            live_out=live_behind(frames, W, H, nf + cnt - 1)))
            nf += cnt
            ns += shown
    return out


def check_images(got, ref, exact):
    """test_gpu_layers._check's rule: all-replace files exact, otherwise at most 1 LSB on at most 0.1 % of the samples."""
    d = np.abs(got.astype(np.int64) - ref.astype(np.int64))
    if exact:
        assert d.max() == 0, (int(d.max()), int((d > 0).sum()))
    else:
        assert d.max() <= 1 and (d > 0).mean() <= 0.001, (int(d.max()), float((d > 0).mean()))
