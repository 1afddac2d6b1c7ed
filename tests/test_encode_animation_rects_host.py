"""CPU tests of animation encode with several rectangles per frame (DESIGN.md §2 "Animation encode", §4.14): the rule that turns a
tile change map into rectangles (csrc/enc_animation.cc: AnimFrameRects, through the test library's hook) against the model of
encode_animation_rects_util on hand-made maps, its invariants on random maps, and the interface: struct sizes, exports, refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import encode_animation_rects_util as RU
from pdn_jpegxl_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 640, 512            # 10 x 8 tiles
FULL = (0, 0, 63, 63)


def both(tiles, w, h, lossless, m, p):
    """The hook's rectangles, asserted equal to the model's."""
    got = RU.hook_frame_rects(api.selftest_lib(), tiles, w, h, lossless, m, p)
    assert got == RU.model_frame_rects(tiles, w, h, lossless, m, p), (lossless, m, p)
    return got


def test_one_tile():
    tiles = RU.map_of(W, H, {(2, 3): (5, 6, 20, 30)})
    assert both(tiles, W, H, True, 4, 0) == [(133, 198, 16, 25)]
    assert both(tiles, W, H, False, 4, 0) == [(128, 192, 24, 32)]


def test_tiles_touching_by_a_corner_are_one_component():
    tiles = RU.map_of(W, H, {(1, 1): (60, 60, 63, 63), (2, 2): (0, 0, 3, 3)})
    assert both(tiles, W, H, True, 4, 0) == [(124, 124, 8, 8)]


def test_tiles_two_apart_are_two_components():
    tiles = RU.map_of(W, H, {(1, 1): FULL, (3, 1): FULL})
    assert both(tiles, W, H, True, 4, 0) == [(64, 64, 64, 64), (192, 64, 64, 64)]


def test_the_closure_swallows_a_component_inside_the_box_of_an_l():
    ell = {(0, y): FULL for y in range(4)}
    ell.update({(x, 3): FULL for x in range(1, 4)})
    inside = {(2, 1): (10, 10, 20, 20)}          # touches no tile of the L, lies in its box
    tiles = RU.map_of(W, H, {**ell, **inside})
    assert both(tiles, W, H, True, 4, 0) == [(0, 0, 256, 256)]
    # ... and a component outside it stays
    tiles = RU.map_of(W, H, {**ell, **inside, (6, 0): FULL})
    assert both(tiles, W, H, True, 4, 0) == [(0, 0, 256, 256), (384, 0, 64, 64)]


def test_three_boxes_and_two_allowed():
    # the cheapest pair merges: the two near each other, whatever their order
    tiles = RU.map_of(W, H, {(0, 0): FULL, (2, 0): FULL, (7, 5): FULL})
    assert both(tiles, W, H, True, 2, 0) == [(0, 0, 192, 64), (448, 320, 64, 64)]
    tiles = RU.map_of(W, H, {(0, 0): FULL, (5, 5): FULL, (7, 5): FULL})
    assert both(tiles, W, H, True, 2, 0) == [(0, 0, 64, 64), (320, 320, 192, 64)]
    # a tie: (0, 1) and (1, 2) cost the same, the first pair merges
    tiles = RU.map_of(W, H, {(0, 0): FULL, (2, 0): FULL, (4, 0): FULL})
    assert both(tiles, W, H, True, 2, 0) == [(0, 0, 192, 64), (256, 0, 64, 64)]
    tiles = RU.map_of(W, H, {(0, 0): FULL, (0, 2): FULL, (0, 4): FULL})
    assert both(tiles, W, H, True, 2, 0) == [(0, 0, 64, 192), (0, 256, 64, 64)]
    # three are allowed: nothing merges
    assert len(both(tiles, W, H, True, 3, 0)) == 3


def test_abutting_boxes_of_equal_extent_merge_at_no_cost():
    """Two components whose tiles do not touch, yet whose boxes abut over their whole height: one box costs no pixel more."""
    a = {(1, 3): FULL, (0, 2): FULL, (0, 1): FULL, (0, 4): FULL, (0, 5): FULL}
    b = {(2, 1): FULL, (3, 2): FULL, (3, 3): FULL, (3, 4): FULL, (2, 5): FULL}
    tiles = RU.map_of(W, H, {**a, **b})
    assert RU.model_frame_rects(RU.map_of(W, H, a), W, H, True, 4, 0) == [(0, 64, 128, 320)]
    assert RU.model_frame_rects(RU.map_of(W, H, b), W, H, True, 4, 0) == [(128, 64, 128, 320)]
    assert both(tiles, W, H, True, 4, 0) == [(0, 64, 256, 320)]


def test_merge_pixels_just_below_and_at_the_cost():
    tiles = RU.map_of(W, H, {(1, 1): FULL, (3, 1): FULL})      # one box would code the 64 x 64 tile between them as well
    assert len(both(tiles, W, H, True, 4, 4095)) == 2
    assert both(tiles, W, H, True, 4, 4096) == [(64, 64, 192, 64)]
    tiles = RU.map_of(W, H, {(1, 1): (3, 3, 3, 3), (3, 1): (7, 9, 7, 9)})   # two pixels: 133 x 7 - 2
    assert len(both(tiles, W, H, True, 4, 133 * 7 - 3)) == 2
    assert both(tiles, W, H, True, 4, 133 * 7 - 2) == [(67, 67, 133, 7)]


@pytest.mark.parametrize("lossless", [True, False], ids=["lossless", "lossy"])
def test_64_and_65_isolated_tiles(lossless):
    w = h = 1280                                               # 20 x 20 tiles: 100 at even coordinates, none touching another
    spots = [(2 * (i % 10), 2 * (i // 10)) for i in range(65)]
    tiles = RU.map_of(w, h, {s: (9, 9, 9, 9) for s in spots[:64]})
    assert len(both(tiles, w, h, lossless, 16, 0)) == 16
    tiles = RU.map_of(w, h, {s: (9, 9, 9, 9) for s in spots})
    want = (9, 9, 18 * 64 + 1, 12 * 64 + 1) if lossless else (8, 8, 18 * 64 + 8, 12 * 64 + 8)
    assert both(tiles, w, h, lossless, 16, 0) == [want]        # too scattered: the one bounding box


def test_lossy_boxes_snap_and_clip_at_the_canvas_edge():
    w, h = 301, 283                                            # neither a multiple of 8; the last tiles are 45 and 27 pixels
    tiles = RU.map_of(w, h, {(4, 4): (40, 20, 44, 26), (0, 0): (1, 1, 2, 2)})
    assert both(tiles, w, h, False, 4, 0) == [(0, 0, 8, 8), (296, 272, 5, 11)]
    assert both(tiles, w, h, True, 4, 0) == [(1, 1, 2, 2), (296, 276, 5, 7)]


@pytest.mark.parametrize("lossless", [True, False], ids=["lossless", "lossy"])
def test_the_empty_table(lossless):
    assert both(RU.empty_map(W, H), W, H, lossless, 4, 4096) == [(0, 0, 1, 1)]
    assert both(RU.empty_map(1, 1), 1, 1, lossless, 2, 0) == [(0, 0, 1, 1)]


def random_map(rng, w, h):
    tiles = RU.empty_map(w, h)
    ny, nx = tiles.shape[:2]
    density = rng.choice([0.03, 0.1, 0.25, 0.6])
    for ty in range(ny):
        for tx in range(nx):
            if rng.random() < density:
                tw, th = min(64, w - 64 * tx), min(64, h - 64 * ty)
                x0, x1 = sorted(int(v) for v in rng.integers(0, tw, 2))
                y0, y1 = sorted(int(v) for v in rng.integers(0, th, 2))
                tiles[ty, tx] = (x0, y0, x1, y1)
    return tiles


@pytest.mark.parametrize("lossless", [True, False], ids=["lossless", "lossy"])
@pytest.mark.parametrize("m", [2, 3, 16])
def test_invariants_on_random_tables(m, lossless):
    rng = np.random.default_rng(1000 * m + lossless)
    for trial in range(200):
        w, h = int(rng.integers(1, 700)), int(rng.integers(1, 600))
        tiles = random_map(rng, w, h)
        p = int(rng.choice([0, 1, 300, 4096, 60000]))
        rects = both(tiles, w, h, lossless, m, p)
        changed = RU.changed_pixels(tiles)
        if not changed:
            assert rects == [(0, 0, 1, 1)]
            continue
        assert len(rects) <= m
        assert rects == sorted(rects, key=lambda r: (r[1], r[0]))
        for x, y, rw, rh in rects:
            assert 0 <= x and 0 <= y and rw >= 1 and rh >= 1 and x + rw <= w and y + rh <= h
        for i, a in enumerate(rects):                          # disjoint
            for b in rects[i + 1:]:
                assert a[0] + a[2] <= b[0] or b[0] + b[2] <= a[0] or a[1] + a[3] <= b[1] or b[1] + b[3] <= a[1], (a, b)
        inside = {r: [] for r in rects}
        for c in changed:                                      # every changed pixel is covered: each tile's box lies in one rectangle
            home = [r for r in rects if r[0] <= c[0] and r[1] <= c[1] and c[2] <= r[0] + r[2] and c[3] <= r[1] + r[3]]
            assert len(home) == 1, c
            inside[home[0]].append(c)
        for r, cs in inside.items():
            assert cs, r                                       # no rectangle without a changed pixel
            if lossless:                                       # tight: every side touches a changed pixel
                assert (min(c[0] for c in cs), min(c[1] for c in cs), max(c[2] for c in cs), max(c[3] for c in cs)) == (r[0], r[1], r[0] + r[2], r[1] + r[3])
            else:                                              # on the grid, or at the canvas edge
                assert r[0] % 8 == 0 and r[1] % 8 == 0 and ((r[0] + r[2]) % 8 == 0 or r[0] + r[2] == w) and ((r[1] + r[3]) % 8 == 0 or r[1] + r[3] == h)
        if len(rects) >= 2:                                    # what is left apart costs more than merge_pixels to join
            area = lambda r: r[2] * r[3]
            for i, a in enumerate(rects):
                for b in rects[i + 1:]:
                    x0, y0 = min(a[0], b[0]), min(a[1], b[1])
                    x1, y1 = max(a[0] + a[2], b[0] + b[2]), max(a[1] + a[3], b[1] + b[3])
                    assert (x1 - x0) * (y1 - y0) - area(a) - area(b) > p


def test_struct_sizes_and_exports():
    hdr = open(os.path.join(ROOT, "include", "jxlfiletypeio.h")).read()
    assert int(re.search(r"static_assert\(sizeof\(JxlHipAnimationOptions\) == (\d+)", hdr).group(1)) == 20 == C.sizeof(api.AnimationOptions)
    assert int(re.search(r"static_assert\(sizeof\(JxlHipAnimationRectOptions\) == (\d+)", hdr).group(1)) == 8 == C.sizeof(api.AnimationRectOptions)
    assert [f[0] for f in api.AnimationRectOptions._fields_] == ["max_rects", "merge_pixels"]
    for name in ("jxlhip_encode_animation", "jxlhip_encoder_animation_rects", "jxlhip_encode_animation_rects", "jxlhip_encoder_animation_frame_rects",
                 "jxlhip_encoder_animation_tiles"):
        assert name in api.EXPORTS and hasattr(api.lib(), name), name
        assert re.search(r"JXLFILETYPEIO_API \w+ %s\(" % name, hdr), name


def test_refusal_messages():
    fn = api.selftest_lib().jxlhip_selftest_animation_rect_options
    fn.restype = C.c_int32
    fn.argtypes = [C.c_int32, C.c_int32, C.POINTER(api.ErrorInfo)]

    def said(m, p):
        err = api.ErrorInfo()
        return fn(m, p, C.byref(err)), err.errorMessage.decode()

    for m, p in ((1, 0), (2, 0), (16, 1 << 30), (1, 4096)):
        assert said(m, p) == (0, "")
    for m in (0, -1, 17, 1 << 20):
        assert said(m, 0) == (1, "the rectangles per frame (max_rects) must be 1..16")
    assert said(4, -1) == (1, "merge_pixels must not be negative")
