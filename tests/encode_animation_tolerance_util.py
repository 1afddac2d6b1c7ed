"""Helpers of the tests of animation encode with a tolerance for "unchanged" (DESIGN.md §2 "Animation encode"): the rule restated in
numpy, independently of the C++ - when a sample counts as changed, the tile map of a frame against the reference canvas R, and how R
follows the rectangles that are written.  The rectangles themselves come from the models the bit rule is tested with
(encode_animation_rects_util.model_frame_rects, encode_animation_util.model_rect).  A tile map is what
api.Encoder.last_animation_tiles returns."""
import ctypes as C
import math

import numpy as np

import encode_animation_rects_util as RU
import encode_animation_util as EU

TILE = RU.TILE
KIND = {"uint8": 0, "uint16": 1, "float16": 2, "float32": 3}      # the sample types as the test library's hook numbers them


def samples_changed(a, b, tolerance):
    """Per sample of two arrays of one dtype: True where it counts as changed under the tolerance."""
    assert a.dtype == b.dtype and a.shape == b.shape
    tol = np.float32(tolerance)                                    # (the interface carries a binary32)
    if a.dtype.kind == "u":
        return np.abs(a.astype(np.int64) - b.astype(np.int64)) > int(math.floor(float(tol)))
    same_bits = EU.bits_of(a) == EU.bits_of(b)
    fa, fb = a.astype(np.float32), b.astype(np.float32)            # (binary16 widens exactly)
    with np.errstate(invalid="ignore", over="ignore"):
        near = np.isfinite(fa) & np.isfinite(fb) & (np.abs(fa - fb) <= tol)
    return ~(same_bits | near)


def tile_map(frame, ref, tolerance):
    """The tile map of a frame (h, w, c) against the reference canvas: per tile the box of the pixels of which some sample changed."""
    h, w = frame.shape[:2]
    d = samples_changed(frame, ref, tolerance).any(axis=2)
    out = RU.empty_map(w, h)
    for ty in range(out.shape[0]):
        for tx in range(out.shape[1]):
            ys, xs = np.nonzero(d[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE])
            if len(xs):
                out[ty, tx] = (xs.min(), ys.min(), xs.max(), ys.max())
    return out


def map_extent(tiles):
    """(x0, y0, x1, y1), inclusive, of everything a tile map marks; None: nothing."""
    boxes = RU.changed_pixels(tiles)
    if not boxes:
        return None
    return min(b[0] for b in boxes), min(b[1] for b in boxes), max(b[2] for b in boxes) - 1, max(b[3] for b in boxes) - 1


def is_key(k, key_interval):
    return k == 0 or (key_interval >= 1 and k % key_interval == 0)


class Model:
    """The whole rule over a stack of frames: .maps[k - 1] the tile map of frame k against R as it stood before frame k, .parts
    [(input frame, x, y, width, height)] per codestream frame, .rects one box per input frame, .shown[k] R after frame k - the source
    of displayed image k."""

    def __init__(self, frames, tolerance, lossless, max_rects=1, merge_pixels=4096, key_interval=0):
        assert tolerance > 0
        self.tolerance, self.lossless, self.max_rects, self.merge_pixels, self.key_interval = tolerance, lossless, max_rects, merge_pixels, key_interval
        h, w = frames[0].shape[:2]
        self.ref = frames[0].copy()                                # R as it stands (a copy is handed out: .shown)
        self.maps, self.parts, self.rects, self.shown = [], [(0, 0, 0, w, h)], [(0, 0, w, h)], [self.ref.copy()]
        for f in frames[1:]:
            self.add(f)

    def add(self, frame):
        """The next frame: measured against R, its rectangles found, R updated."""
        k = len(self.shown)
        h, w = frame.shape[:2]
        tiles = tile_map(frame, self.ref, self.tolerance)
        self.maps.append(tiles)
        box = EU.model_rect(k, map_extent(tiles), w, h, self.lossless, self.key_interval)
        if is_key(k, self.key_interval) or self.max_rects == 1:
            rects = [box]
        else:
            rects = RU.model_frame_rects(tiles, w, h, self.lossless, self.max_rects, self.merge_pixels)
        for x, y, rw, rh in rects:                                 # R takes what a decoder replaces
            self.ref[y:y + rh, x:x + rw] = frame[y:y + rh, x:x + rw]
        self.parts += [(k,) + tuple(r) for r in rects]
        self.rects.append(box)
        self.shown.append(self.ref.copy())


def worst_error(shown, frames):
    """max |shown - frame| over all samples and frames (integers; floats: over the finite samples)."""
    worst = 0.0
    for s, f in zip(shown, frames):
        if f.dtype.kind == "u":
            worst = max(worst, float(np.abs(s.astype(np.int64) - f.astype(np.int64)).max()))
        else:
            a, b = s.astype(np.float32), f.astype(np.float32)
            ok = np.isfinite(a) & np.isfinite(b)
            worst = max(worst, float(np.abs(a[ok] - b[ok]).max()) if ok.any() else 0.0)
    return worst


# ---------------------------------------------------------------- the prototype's stack: a sprite, a toggling block, noise
def sprite_stack(n=8, w=150, h=70, nch=4, noise=0, seed=5):
    """n frames (h, w, nch) uint8: a flat background, a flat 12 x 9 sprite moving right and down, a 6 x 5 block in the far corner that
    toggles every other frame; `noise`: uniform in [-noise, noise], new for every frame and sample."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        f = np.full((h, w, nch), 90, np.int64)
        x, y = 8 + 5 * k, 6 + 3 * k
        f[y:y + 9, x:x + 12] = 170
        if k % 2:
            f[h - 7:h - 2, w - 9:w - 3] = 30
        if noise:
            f += rng.integers(-noise, noise + 1, f.shape)
        out.append(f.astype(np.uint8))
    return out


# ---------------------------------------------------------------- the test library's hooks
def hook_sample_changed(lib, dtype, a_bits, b_bits, tolerance):
    fn = lib.jxlhip_selftest_animation_sample_changed
    fn.restype = None
    fn.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p]
    a = np.ascontiguousarray(a_bits, np.uint32)
    b = np.ascontiguousarray(b_bits, np.uint32)
    out = np.zeros(len(a), np.uint8)
    fn(KIND[np.dtype(dtype).name], a.ctypes.data, b.ctypes.data, len(a), float(tolerance), out.ctypes.data)
    return out.astype(bool)


def hook_tolerance_refusal(lib, tolerance):
    from pdn_jpegxl_amd import api
    fn = lib.jxlhip_selftest_animation_tolerance
    fn.restype = C.c_int32
    fn.argtypes = [C.c_float, C.POINTER(api.ErrorInfo)]
    err = api.ErrorInfo()
    return fn(float(tolerance), C.byref(err)), err.errorMessage.decode()
