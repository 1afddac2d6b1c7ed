"""ClampedGradientSmall (csrc/modular_rules.h), the median form of predictor 5 that the one-pass alpha decode uses on its u8 rows: equal
to ClampedGradient32, and to the rule written out here, wherever W + N - NW does not overflow."""
import ctypes as C
import itertools

import numpy as np

from pdn_jpegxl_amd import api


def both(wnnw):
    L = api.selftest_lib()
    L.jxlhip_selftest_gradient_small.restype = None
    L.jxlhip_selftest_gradient_small.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    wnnw = np.ascontiguousarray(wnnw, np.int32)
    n = len(wnnw)
    small, g32 = np.zeros(n, np.int32), np.zeros(n, np.int32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    L.jxlhip_selftest_gradient_small(n, p(wnnw), p(small), p(g32))
    return small, g32


def rule(wnnw):
    w, n, nw = (wnnw[:, i].astype(np.int64) for i in range(3))
    return np.clip(w + n - nw, np.minimum(w, n), np.maximum(w, n))


def test_every_small_neighbourhood_and_random_large_ones():
    edge = [0, 1, 2, 3, 63, 64, 127, 128, 129, 200, 253, 254, 255]
    cases = [np.array(list(itertools.product(edge, repeat=3)))]
    rng = np.random.default_rng(5)
    cases.append(rng.integers(0, 256, (20000, 3)))
    # a sample outside 0 .. 255 is followed by up to fifteen more of its period: West may be anything a residual of 16 bits adds up to
    cases.append(np.stack([rng.integers(-(1 << 20), 1 << 20, 20000), rng.integers(0, 256, 20000), rng.integers(0, 256, 20000)], 1))
    cases.append(rng.integers(-(1 << 29), 1 << 29, (20000, 3)))
    for c in cases:
        small, g32 = both(c)
        want = rule(np.asarray(c))
        assert (small == want).all() and (g32 == want).all()
