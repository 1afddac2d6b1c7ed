"""CPU tests of animation encode with a tolerance for "unchanged" (DESIGN.md §2 "Animation encode", §4.14): the refusals, the rule of
one sample (csrc/enc_animation.h: AnimSampleChanged, through the test library's hook) against the numpy rule of
encode_animation_tolerance_util on edge values, the interface, and the invariants of the model itself - the bound against what is
shown, noise that codes nothing, a ramp that is coded every fourth frame."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import encode_animation_rects_util as RU
import encode_animation_tolerance_util as TU
import encode_animation_util as EU
from pdn_jpegxl_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refusals():
    lib = api.selftest_lib()
    for t in (0.0, -0.0, 0.5, 6.0, 65535.0, 1e30, 1e-45):
        assert TU.hook_tolerance_refusal(lib, t) == (0, ""), t
    for t in (-1.0, -1e-30, -1e30):
        assert TU.hook_tolerance_refusal(lib, t) == (1, "the tolerance must not be negative"), t
    for t in (float("nan"), float("inf"), float("-inf")):
        assert TU.hook_tolerance_refusal(lib, t) == (1, "the tolerance must be a finite number"), t


def test_struct_size_and_exports():
    hdr = open(os.path.join(ROOT, "include", "jxlfiletypeio.h")).read()
    assert int(re.search(r"static_assert\(sizeof\(JxlHipAnimationChangeOptions\) == (\d+)", hdr).group(1)) == 4 == C.sizeof(api.AnimationChangeOptions)
    assert [f[0] for f in api.AnimationChangeOptions._fields_] == ["tolerance"]
    name = "jxlhip_encode_animation_changes"
    assert name in api.EXPORTS and hasattr(api.lib(), name)
    assert re.search(r"JXLFILETYPEIO_API \w+ %s\(" % name, hdr)


def both(dtype, a, b, tolerance):
    """The hook's verdicts on the samples a against b, asserted equal to numpy's."""
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    want = TU.samples_changed(a, b, tolerance)
    got = TU.hook_sample_changed(api.selftest_lib(), dtype, EU.bits_of(a), EU.bits_of(b), tolerance)
    assert (got == want).all(), (np.dtype(dtype).name, tolerance, a[got != want], b[got != want])
    return got.tolist()


@pytest.mark.parametrize("dtype,top", [(np.uint8, 255), (np.uint16, 65535)], ids=["u8", "u16"])
def test_integer_samples_at_and_past_the_tolerance(dtype, top):
    for tol in (1, 3, 6, 100):
        a = [100, 100, 100 + tol, 100 + tol + 1, 0, top, 0, top - tol, top - tol - 1]
        b = [100 + tol, 100 + tol + 1, 100, 100, tol, top - tol, tol + 1, top, top]
        assert both(dtype, a, b, tol) == [False, True, False, True, False, False, True, False, True]
    # fractional tolerances: floor decides - 3.9 is 3, 0.99 is the bit rule
    assert both(dtype, [10, 10, 10], [13, 14, 6], 3.9) == [False, True, True]
    assert both(dtype, [10, 10, 10], [10, 11, 9], 0.99) == [False, True, True]
    # a tolerance as large as the range, or far larger: nothing is changed
    assert both(dtype, [0, top, 5], [top, 0, 5], float(top)) == [False, False, False]
    assert both(dtype, [0, top], [top, 0], 1e30) == [False, False]
    assert both(dtype, [0, top], [top, 0], top - 1) == [True, True]
    # every pair of a small grid against the numpy rule
    v = np.arange(0, top + 1, max(1, top // 97), dtype=np.int64)
    a, b = np.meshgrid(v, v)
    both(dtype, a.ravel(), b.ravel(), 7.5)


def bits(dtype, *patterns):
    u = np.uint16 if np.dtype(dtype).itemsize == 2 else np.uint32
    return np.array(patterns, u).view(dtype)


@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=["f16", "f32"])
def test_float_samples(dtype):
    half = np.dtype(dtype).itemsize == 2
    nan1, nan2 = (0x7E01, 0x7E02) if half else (0x7FC00001, 0x7FC00002)
    pinf, ninf = (0x7C00, 0xFC00) if half else (0x7F800000, 0xFF800000)
    pzero, nzero = (0x0000, 0x8000) if half else (0x00000000, 0x80000000)
    one = 0x3C00 if half else 0x3F800000
    # exactly the tolerance, and one step of 1/64 past it (all exactly representable)
    assert both(dtype, [1.0, 1.0, 2.25, 2.25, -0.125], [1.25, 1.265625, 2.0, 1.984375, 0.125], 0.25) == [False, True, False, True, False]
    # +0 / -0 are unchanged under a tolerance; equal NaN patterns are; other NaNs, and infinities against anything else, are changed
    a = bits(dtype, pzero, nan1, nan1, nan1, pinf, pinf, pinf, ninf, one, nan1, pzero)
    b = bits(dtype, nzero, nan1, nan2, one, pinf, ninf, one, ninf, pinf, pinf, pzero)
    assert both(dtype, a, b, 0.25) == [False, False, True, True, False, True, True, False, True, True, False]
    assert both(dtype, a, b, 1e30) == [False, False, True, True, False, True, True, False, True, True, False]
    # a tiny tolerance still forgives the sign of zero and nothing else
    assert both(dtype, bits(dtype, pzero, one), bits(dtype, nzero, one + 1), 1e-30) == [False, True]
    # the largest finite values: their difference overflows binary32 only for binary32 (changed); binary16 is widened first
    big = np.array([np.finfo(dtype).max, -np.finfo(dtype).max], dtype)
    assert both(dtype, big, big[::-1], 1e30) == ([False, False] if half else [True, True])


def test_binary16_is_widened_before_the_subtraction():
    # 2048 and 2050 are neighbours in binary16: their difference is exactly 2 in binary32
    assert both(np.float16, [2048.0, 2048.0], [2050.0, 2050.0], 2.0) == [False, False]
    assert both(np.float16, [2048.0], [2050.0], 1.999) == [True]
    # subnormals widen exactly too: 2^-24, 3 * 2^-24 and the largest, 1023 * 2^-24, against a tolerance of 2 * 2^-24
    sub = bits(np.float16, 0x0001, 0x0003, 0x03FF)
    assert both(np.float16, sub, sub[::-1], 2.0 ** -23) == [True, False, True]
    assert both(np.float16, bits(np.float16, 0x0001), bits(np.float16, 0x0003), 2.0 ** -23) == [False]
    assert both(np.float16, bits(np.float16, 0x0001), bits(np.float16, 0x0004), 2.0 ** -23) == [True]
    # every binary16 pattern against its neighbour 37 patterns on, against numpy
    a = np.arange(0, 65536, dtype=np.uint32)
    b = (a + 37) % 65536
    both(np.float16, a.astype(np.uint16).view(np.float16), b.astype(np.uint16).view(np.float16), 0.01)


# ---------------------------------------------------------------- the model's own invariants
@pytest.mark.parametrize("lossless", [True, False], ids=["lossless", "lossy"])
@pytest.mark.parametrize("max_rects", [1, 4])
def test_noise_within_the_tolerance_codes_what_the_clean_stack_codes(lossless, max_rects):
    clean, noisy = TU.sprite_stack(noise=0), TU.sprite_stack(noise=3)
    m = TU.Model(noisy, 6, lossless, max_rects, 4096)
    assert m.parts == RU.model_animation_frame_rects(clean, lossless, max_rects, 4096)
    assert m.rects == EU.model_rects(clean, lossless)
    assert TU.worst_error(m.shown, noisy) <= 6
    if max_rects == 4:
        assert [sum(1 for p in m.parts if p[0] == k) for k in range(len(noisy))] == [1] + [2] * (len(noisy) - 1)
    # ... and under the bit rule every frame of the noisy stack is (nearly) the canvas
    assert all(r[2] * r[3] > 0.9 * 150 * 70 for r in EU.model_rects(noisy, lossless)[1:])


def test_the_bound_holds_against_what_is_shown_on_random_walks():
    rng = np.random.default_rng(3)
    for dtype, tol, step, lo in ((np.uint8, 4, 3, 60), (np.uint16, 300.5, 200, 20000), (np.float32, 0.25, 0.125, 60), (np.float16, 0.25, 0.125, 60)):
        f = rng.integers(lo, lo + 60, (70, 150, 3)).astype(np.float64)
        frames = []
        for k in range(8):
            f = f + rng.integers(-1, 2, f.shape) * step * (rng.random(f.shape) < 0.3)
            frames.append(f.astype(dtype))
        for lossless, m in ((True, 1), (False, 4)):
            model = TU.Model(frames, tol, lossless, m, 0)
            assert TU.worst_error(model.shown, frames) <= tol
            assert len(model.maps) == 7 and len(model.shown) == 8


def test_a_ramp_is_coded_every_fourth_frame():
    base = np.full((70, 150, 4), 50, np.uint8)
    frames = []
    for k in range(9):
        f = base.copy()
        f[20:30, 40:60] += k
        frames.append(f)
    m = TU.Model(frames, 3, True)
    region = (40, 20, 20, 10)
    assert m.rects == [(0, 0, 150, 70)] + [region if k % 4 == 0 else (0, 0, 1, 1) for k in range(1, 9)]
    assert EU.model_rects(frames, True)[1:] == [region] * 8         # the bit rule codes every frame
    assert TU.worst_error(m.shown, frames) == 3


def test_the_reference_follows_the_boxes_not_the_pixels():
    """A pixel that moved within the tolerance inside a coded box is shown as it is now: the next frame is measured against that."""
    f0 = np.full((70, 150, 1), 100, np.uint8)
    f1 = f0.copy()
    f1[10:13, 10:13] = 150
    f1[11, 11] = 104
    f2 = f1.copy()
    f2[11, 11] = 97
    m = TU.Model([f0, f1, f2], 4, True)
    assert m.rects[1:] == [(10, 10, 3, 3), (11, 11, 1, 1)]          # (against a per-pixel reference, 97 is 3 from 100: unchanged)
    assert m.shown[1][11, 11, 0] == 104
