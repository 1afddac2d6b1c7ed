"""Helpers of the tests of animation encode with several rectangles per frame: the rectangle rule of DESIGN.md §2 "Animation encode"
written out independently of csrc/enc_animation.cc (sets of tiles and lists of boxes, no shared code), and what changed per 64 x 64
tile by numpy.  A tile map is a (tiles down, tiles across, 4) uint8 array of x0, y0, x1, y1 - inclusive, relative to the tile - with
255 everywhere for a tile in which nothing changed: what api.Encoder.last_animation_tiles returns."""
import ctypes as C

import numpy as np

import encode_animation_util as EU

TILE = 64
MAX_COMPONENTS = 64


def tiles_across(pixels):
    return (pixels + TILE - 1) // TILE


def empty_map(w, h):
    return np.full((tiles_across(h), tiles_across(w), 4), 255, np.uint8)


def tile_boxes(a, b):
    """The tile map of two frames (h, w, c): per tile the box of the pixels of which some sample differs in its bits."""
    h, w = a.shape[:2]
    d = (EU.bits_of(a) != EU.bits_of(b)).any(axis=2)
    out = empty_map(w, h)
    for ty in range(out.shape[0]):
        for tx in range(out.shape[1]):
            ys, xs = np.nonzero(d[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE])
            if len(xs):
                out[ty, tx] = (xs.min(), ys.min(), xs.max(), ys.max())
    return out


def map_of(w, h, boxes):
    """A hand-made tile map: {(tx, ty): (x0, y0, x1, y1)}."""
    out = empty_map(w, h)
    for (tx, ty), box in boxes.items():
        out[ty, tx] = box
    return out


def changed_pixels(tiles):
    """The canvas boxes (x0, y0, x1, y1), exclusive ends, of the non-empty tiles."""
    out = []
    for ty, tx in zip(*np.nonzero(tiles[:, :, 0] != 255)):
        x0, y0, x1, y1 = (int(v) for v in tiles[ty, tx])
        out.append((tx * TILE + x0, ty * TILE + y0, tx * TILE + x1 + 1, ty * TILE + y1 + 1))
    return out


def _union(a, b):
    return (min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3]))


def _area(a):
    return (a[2] - a[0]) * (a[3] - a[1])


def _share(a, b):
    return max(a[0], b[0]) < min(a[2], b[2]) and max(a[1], b[1]) < min(a[3], b[3])


def _closure(boxes):
    boxes = list(boxes)
    while True:
        hit = next(((i, j) for i in range(len(boxes)) for j in range(i + 1, len(boxes)) if _share(boxes[i], boxes[j])), None)
        if hit is None:
            return boxes
        i, j = hit
        boxes[i] = _union(boxes[i], boxes[j])
        del boxes[j]


def _in_order(boxes):
    return sorted(boxes, key=lambda b: (b[1], b[0]))


def model_frame_rects(tiles, w, h, lossless, max_rects, merge_pixels):
    """[(x, y, width, height)] of a frame that is no key frame, by the rule."""
    left = {(int(tx), int(ty)) for ty, tx in zip(*np.nonzero(tiles[:, :, 0] != 255))}
    if not left:
        return [(0, 0, 1, 1)]
    tile_box = {}
    for tx, ty in left:
        x0, y0, x1, y1 = (int(v) for v in tiles[ty, tx])
        tile_box[(tx, ty)] = (tx * TILE + x0, ty * TILE + y0, tx * TILE + x1 + 1, ty * TILE + y1 + 1)
    boxes = []
    while left:                                   # components: tiles that touch by a side or a corner
        front = [left.pop()]
        box = tile_box[front[0]]
        while front:
            tx, ty = front.pop()
            for n in [(tx + dx, ty + dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1)]:
                if n in left:
                    left.remove(n)
                    front.append(n)
                    box = _union(box, tile_box[n])
        if not lossless:
            box = (box[0] // 8 * 8, box[1] // 8 * 8, min(w, -(-box[2] // 8) * 8), min(h, -(-box[3] // 8) * 8))
        boxes.append(box)
    boxes = _closure(boxes)
    if len(boxes) > MAX_COMPONENTS:
        all_of_them = boxes[0]
        for b in boxes:
            all_of_them = _union(all_of_them, b)
        boxes = [all_of_them]
    boxes = _in_order(boxes)
    while len(boxes) >= 2:
        cost, i, j = min((_area(_union(boxes[i], boxes[j])) - _area(boxes[i]) - _area(boxes[j]), i, j)
                         for i in range(len(boxes)) for j in range(i + 1, len(boxes)))
        if len(boxes) <= max_rects and cost > merge_pixels:
            break
        boxes[i] = _union(boxes[i], boxes[j])
        del boxes[j]
        boxes = _in_order(_closure(boxes))
    return [(b[0], b[1], b[2] - b[0], b[3] - b[1]) for b in boxes]


def model_animation_frame_rects(frames, lossless, max_rects, merge_pixels, key_interval=0):
    """[(input frame, x, y, width, height)] per codestream frame of an animation: key frames whole, the others by the rule."""
    h, w = frames[0].shape[:2]
    out = []
    for k in range(len(frames)):
        if k == 0 or (key_interval >= 1 and k % key_interval == 0):
            out.append((k, 0, 0, w, h))
        elif max_rects == 1:
            out.append((k,) + EU.model_rect(k, EU.changed_box(frames[k - 1], frames[k]), w, h, lossless))
        else:
            out += [(k,) + r for r in model_frame_rects(tile_boxes(frames[k - 1], frames[k]), w, h, lossless, max_rects, merge_pixels)]
    return out


def hook_frame_rects(lib, tiles, w, h, lossless, max_rects, merge_pixels):
    """jxlhip_selftest_animation_frame_rects of the test library `lib` on a tile map."""
    fn = lib.jxlhip_selftest_animation_frame_rects
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32]
    assert tiles.shape == (tiles_across(h), tiles_across(w), 4) and tiles.dtype == np.uint8
    words = np.ascontiguousarray(tiles).view(np.uint32).reshape(-1).copy()
    cap = 128
    out = (C.c_int32 * (4 * cap))()
    n = fn(words.ctypes.data, w, h, 1 if lossless else 0, max_rects, merge_pixels, out, cap)
    assert 0 < n <= cap
    return [tuple(out[4 * i:4 * i + 4]) for i in range(n)]
