"""Helpers of the animation encode tests: the model of the rectangle rules, what changed between two frames by numpy,
and a walk over the frames of an encoded file."""
import numpy as np

import layer_util as LU

_UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def bits_of(a):
    """The samples as unsigned integers of their size: what "differs" means."""
    return np.ascontiguousarray(a).view(_UINT[a.dtype.itemsize])


def changed_box(a, b):
    """(x0, y0, x1, y1), inclusive, of the pixels of which some sample differs in its bits; None: none does."""
    d = (bits_of(a) != bits_of(b)).any(axis=2)
    if not d.any():
        return None
    ys, xs = np.nonzero(d)
    return int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())


def model_rect(k, ext, w, h, lossless, key_interval=0):
    """The rectangle (x, y, width, height) frame k is written as.  ext: changed_box against frame k - 1."""
    if k == 0 or (key_interval >= 1 and k % key_interval == 0):
        return (0, 0, w, h)
    if ext is None:
        return (0, 0, 1, 1)
    x0, y0, x1, y1 = ext[0], ext[1], ext[2] + 1, ext[3] + 1
    if not lossless:
        x0, y0 = x0 // 8 * 8, y0 // 8 * 8
        x1, y1 = min(w, (x1 + 7) // 8 * 8), min(h, (y1 + 7) // 8 * 8)
    return (x0, y0, x1 - x0, y1 - y0)


def model_rects(frames, lossless, key_interval=0):
    h, w = frames[0].shape[:2]
    return [model_rect(k, changed_box(frames[k - 1], frames[k]) if k else None, w, h, lossless, key_interval) for k in range(len(frames))]


def codestream(file):
    return file[file.index(b"jxlc") + 4:]


def walk_frames(file, frame_files):
    """The frame headers of an animated file whose frame k carries, from its TOC on, the bytes of the single-frame file frame_files[k]
    from its TOC on (asserted: that is how the next frame is found).  Returns (ImageInfo, [FrameHeader])."""
    cs = codestream(file)
    info = LU.read_image_header(cs)
    canvas = (info.xsize, info.ysize)
    pos, out = info.frame_start, []
    for k, ref in enumerate(frame_files):
        h, end = LU.read_frame_header(cs, pos, info, canvas)
        assert not LU.BitReader(cs, end).b(), "frame %d: permuted TOC" % k
        toc = (end + 1 + 7) // 8
        rcs = codestream(ref)
        _, _, rend = LU.frame_of(rcs)
        body = rcs[(rend + 1 + 7) // 8:]
        assert cs[toc:toc + len(body)] == body, "frame %d differs from save_pixels of its rectangle from the TOC on" % k
        pos = toc + len(body)
        out.append(h)
    assert pos == len(cs), "bytes behind the last frame"
    return info, out
