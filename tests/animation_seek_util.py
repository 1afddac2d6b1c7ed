"""Helpers of the seek and thumbnail tests of animations: the host logic through the test library
(jxlhip_selftest_animation_seek_plan), the model of the rules it is checked against, written from the frame
list the test built, and a file with entry points in the middle."""
import ctypes as C

import numpy as np

import animation_util as AU
from pdn_jpegxl_amd import api
from test_gpu_layers import F

SEEK, NEXT, NEXT_REDUCED = 0, 1, 2
CHUNK_KEYS = ("op", "first", "count", "first_shown", "shown", "live_in", "live_out", "first_stored", "stored", "step")


class SeekPlan:
    pass


def seek_plan(data, ops, chunk_frames=0, scratch_budget=0):
    """ops: tuples (SEEK, j), (NEXT, n) or (NEXT_REDUCED, n, step); n <= 0: all that is left.  Returns an object with `entry_points`,
    `results` (per operation: (accepted, codestream frame, displayed image) behind it) and `chunks` (dicts of CHUNK_KEYS plus
    `stores`, the displayed images the chunk stores)."""
    L = api.selftest_lib()
    fn = L.jxlhip_selftest_animation_seek_plan
    fn.restype = C.c_size_t
    fn.argtypes = [C.c_char_p, C.c_size_t, C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int64), C.c_size_t, C.POINTER(C.c_int32),
                   C.POINTER(api.ErrorInfo)]
    flat = []
    for op in ops:
        flat += list(op) + [0] * (3 - len(op))
    cap = 1 << 16
    out = (C.c_int64 * cap)()
    arr = (C.c_int32 * max(1, len(flat)))(*flat)
    st, err = C.c_int32(0), api.ErrorInfo()
    n = fn(data, len(data), chunk_frames, scratch_budget, arr, len(ops), out, cap, C.byref(st), C.byref(err))
    if n == 0:
        raise api.FormatError(api.DECODER_STATUS[st.value], err.errorMessage.decode("ascii", "replace"))
    v = list(out[:n])
    p = SeekPlan()
    ne = v[0]
    p.entry_points = v[1:1 + ne]
    at = 1 + ne
    p.results = [tuple(v[at + 3 * i:at + 3 * i + 3]) for i in range(len(ops))]
    at += 3 * len(ops)
    nchunks = v[at]
    at += 1
    k = len(CHUNK_KEYS)
    p.chunks = [dict(zip(CHUNK_KEYS, v[at + k * i:at + k * i + k])) for i in range(nchunks)]
    assert at + k * nchunks == n
    for c in p.chunks:
        c["stores"] = [c["first_stored"] + i * c["step"] for i in range(c["stored"])]
    return p


# ---------------------------------------------------------------- the model
def first_frame(frames, j):
    """The first codestream frame of displayed image j (j == the number of images: the number of frames)."""
    done = [k for k, s in enumerate(AU.shows(frames)) if s >= 0]
    return 0 if j == 0 else (len(frames) if j >= len(done) else done[j - 1] + 1)


def model_entry_points(frames, W, H):
    total = max(AU.shows(frames)) + 1
    return [j for j in range(total) if j == 0 or AU.live_behind(frames, W, H, first_frame(frames, j) - 1) == 0]


def model_run(frames, W, H, ops, chunk_frames=0, scratch=None, budget=None):
    """(results, chunks) of the operations by the rules of the issue: a seek resumes at the latest entry point e <= j unless the decode
    stands at an image in [e, j]; the images asked for and the ones in front of them travel in the same chunks (AU.model_chunks' cuts);
    a chunk stores the selected images it completes."""
    sh = AU.shows(frames)
    total = max(sh) + 1
    done = [k for k, s in enumerate(sh) if s >= 0]
    entries = model_entry_points(frames, W, H)
    cap = min(chunk_frames, AU.MAX_CHUNK_FRAMES) if chunk_frames >= 1 else AU.MAX_CHUNK_FRAMES
    image_of = lambda k: sum(1 for d in done if d < k)
    nf = ns = 0
    results, chunks = [], []
    for i, op in enumerate(ops):
        if op[0] == SEEK:
            j = op[1]
            ok = 0 <= j <= total
            if ok and j != ns:
                e = max(x for x in entries if x <= j)
                if not e <= image_of(nf) <= j:
                    nf = first_frame(frames, e)
                ns = j
            results.append((int(ok), nf, ns))
            continue
        step = op[2] if op[0] == NEXT_REDUCED else 1
        if step < 1:
            results.append((0, nf, ns))
            continue
        left = -(-(total - ns) // step)
        n = max(0, left if op[1] <= 0 else min(op[1], left))
        sel = [ns + q * step for q in range(n)]
        while n and image_of(nf) <= sel[-1]:
            cnt = used = 0
            shown = []
            while nf + cnt < len(frames) and cnt < cap:
                if budget is not None and cnt > 0 and used + scratch[nf + cnt] > budget:
                    break
                if budget is not None:
                    used += scratch[nf + cnt]
                cnt += 1
                if sh[nf + cnt - 1] >= 0:
                    shown.append(sh[nf + cnt - 1])
                    if shown[-1] >= sel[-1]:
                        break
            chunks.append(dict(op=i, first=nf, count=cnt, shown=len(shown), live_in=AU.live_behind(frames, W, H, nf - 1) if nf else 0,
                               live_out=AU.live_behind(frames, W, H, nf + cnt - 1), stores=[s for s in shown if s in sel]))
            nf += cnt
        ns = min(total, ns + n * step)
        results.append((1, nf, ns))
    return results, chunks


def brief(chunks):
    """The fields the model states, of the library's chunks."""
    return [{k: c[k] for k in ("op", "first", "count", "shown", "live_in", "live_out", "stores")} for c in chunks]


# ---------------------------------------------------------------- a file with entry points in the middle
KW, KH = 21, 10


def keyed_frames(bits=8, nch=4, seed=17, w=KW, h=KH):
    """Twelve displayed images of fourteen frames on a w x h canvas, entry points 0, 4 and 8: every fourth image replaces the whole
    canvas and is saved to slot 1; the three behind it blend a crop onto slot 1 and are saved there.  Image 6 has a zero-duration layer
    in front of it and image 10 one that goes through slot 2."""
    rng = np.random.default_rng(seed)
    px = lambda ww, hh: rng.integers(0, 1 << bits, (hh, ww, nch), dtype=np.uint8 if bits <= 8 else np.uint16)
    frames = []
    for j in range(12):
        if j % 4 == 0:
            frames.append(F(px(w, h), crop=False, duration=1, save=1))
            continue
        if j == 6:
            frames.append(F(px(5, 4), x0=1, y0=2, mode=1, source=1, save=1))
        if j == 10:
            frames.append(F(px(7, 3), x0=-2, y0=5, mode=2, source=1, save=2))
        src = 2 if j == 10 else 1
        frames.append(F(px(w // 2 + 1, h // 2 + 1), x0=(3 * j) % (w // 2 + 1) - 1, y0=j % (h // 2 + 1) - 1, mode=2 if nch in (2, 4) else 1, source=src,
                        duration=1, save=1))
    return frames


KEYED_ENTRY_POINTS = [0, 4, 8]
