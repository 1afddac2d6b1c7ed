"""CPU checks of the reduced-size decode's helpers: the size rule, the cell means, and that the colour reference reads the oracle's LF
dump in the right channel order and scale ("Reduced-size decode")."""
import numpy as np
import pytest

import downscale_util as DU
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth


@pytest.mark.parametrize("n,want", [(1, 1), (7, 1), (8, 1), (9, 2), (256, 32), (257, 33)])
def test_reduced_size(n, want):
    assert api.reduced_size(n, 8, 8) == (want, 1)
    assert api.reduced_size(8, n, 8) == (1, want)
    assert api.reduced_size(n, n, 1) == (n, n)
    with pytest.raises(ValueError):
        api.reduced_size(n, n, 4)


@pytest.mark.parametrize("orientation", range(1, 9))
def test_reduced_size_follows_the_displayed_size(oracle, orientation):
    """reduced_size takes what peek reports: for orientations 5..8 the sides are swapped before the division, as in the decode."""
    w, h = 23, 9
    info = api.peek(oracle.encode(synth(w, h, 1), lossless=True, orientation=orientation))
    assert (info.width, info.height) == ((h, w) if orientation >= 5 else (w, h))
    assert api.reduced_size(info.width, info.height, 8) == ((2, 3) if orientation >= 5 else (3, 2))


def test_box_mean_int_known_answers():
    assert DU.box_mean_int(np.array([[7]], np.uint8)).tolist() == [[7]]
    a = np.zeros((9, 9), np.uint8)
    a[:8, :8] = 10
    a[:8, 8] = 20
    a[8, :8] = 30
    a[8, 8] = 40
    assert DU.box_mean_int(a).tolist() == [[10, 20], [30, 40]]        # edge cells of 8x1, 1x8 and 1x1 pixels
    half = np.zeros((8, 8), np.uint8)
    half.flat[:32] = 1                                                 # sum 32 of 64: exactly on the half, rounds up
    assert DU.box_mean_int(half).tolist() == [[1]]
    half.flat[31] = 0                                                  # sum 31: just below
    assert DU.box_mean_int(half).tolist() == [[0]]
    odd = np.array([[1, 2, 2]], np.uint16)                             # n = 3: (5 + 1) // 3 = 2
    assert DU.box_mean_int(odd).tolist() == [[2]] and DU.box_mean_int(odd).dtype == np.uint16
    top = np.full((8, 8, 2), 65535, np.uint16)                         # 64 * 65535 does not wrap
    assert (DU.box_mean_int(top) == 65535).all() and DU.box_mean_int(top).shape == (1, 1, 2)
    assert DU.box_mean_float(np.array([[0.5, 1.0, 3.0]], np.float32)).tolist() == [[1.5]]


def test_reference_colour_reads_the_lf_dump(oracle):
    """A flat colour: every pixel of the full decode is (up to the codec's own error) the colour of its cell's LF sample, so the
    reference of rule 1 must agree with the oracle's pixels at every 8th position within 1 LSB.  A swapped channel or a wrong scale
    of the dump would be off by tens of steps for this colour."""
    w, h = 40, 24
    img = np.empty((h, w, 3), np.uint8)
    img[...] = (200, 90, 30)
    od = oracle.decode(oracle.encode(img, distance=1.0), want_dump=True)
    ref = DU.reference_colour(od, np.uint8)
    assert ref.shape == (3, 5, 3)
    d = np.abs(ref.astype(int) - od.pixels[::8, ::8, :3].astype(int))
    print("max difference %d LSB" % d.max())
    assert d.max() <= 1
