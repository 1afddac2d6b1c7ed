"""What the GPU tests of the chroma-from-luma fit (test_gpu_cfl_fit.py) rest on, shown on the oracle alone: its fitted maps
(side_info=dict(cfl="fitted"), oracle/jxo_enc.cc) save bytes and do not cost pixels on the test pictures, and the pictures reach the
edges of the rule - both clamps, a tile without any dequantised Y, a second LF group, all-zero maps."""
import numpy as np
import pytest

import cfl_util as U

# (picture, measured fitted / zero ratio over distances 1.0, 3.0 and the three strategy modes, asserted bound)
RATIOS = [(("tex", 192, 128, 3), 0.74, 0.80), (("tex", 65, 130, 5), 0.78, 0.85), (("synth", 512, 384, 7), 0.971, 0.99)]


@pytest.mark.parametrize("mode", U.MODES)
@pytest.mark.parametrize("distance", [1.0, 3.0])
@pytest.mark.parametrize("pic,measured,bound", RATIOS, ids=[p[0][0] + "%dx%d" % p[0][1:3] for p in RATIOS])
def test_fitted_maps_save_bytes_and_keep_the_pixels(oracle, pic, measured, bound, distance, mode):
    fitted, zero = U.oracle_file(*pic, distance, mode, True), U.oracle_file(*pic, distance, mode, False)
    ratio = len(fitted) / len(zero)
    print("bytes fitted / zero = %.4f" % ratio)
    assert ratio <= bound
    img = U._PICTURES[pic[0]](*pic[1:])
    p_fit, p_zero = U.psnr(oracle.decode(fitted).pixels, img), U.psnr(oracle.decode(zero).pixels, img)
    print("PSNR fitted %.3f dB, zero %.3f dB" % (p_fit, p_zero))
    assert p_fit >= p_zero


def test_the_texture_clamps_ytob_in_every_tile():
    ytox, ytob = U.maps_of(U.oracle_dump("tex", 192, 128, 3, 1.0, 0))
    assert ytob.shape == (2, 3) and (ytob == -128).all() and (ytox != 0).all()


def test_a_second_lf_group_of_one_tile_column_with_both_clamps():
    d = U.oracle_dump("synth", 2112, 72, 11, 1.0, 1)
    ytox, ytob = U.maps_of(d)
    assert ytox.shape == (2, 33)                                   # 33 x 2 tiles: tile column 32 lies in the second LF group
    assert (ytox[:, 32] != 0).any() and (ytob[:, 32] != 0).any()
    both = np.concatenate([ytox.ravel(), ytob.ravel()])
    assert both.min() == -128 and both.max() == 127


def test_a_tile_without_dequantised_y_keeps_zero_beside_fitted_ones():
    ytox, ytob = U.maps_of(U.oracle_dump("tex", 65, 130, 5, 3.0, 0))
    assert ytox.shape == (3, 2)
    empty = (ytox == 0) & (ytob == 0)
    assert empty.any() and not empty.all()


@pytest.mark.parametrize("img", [U.flat64(), U.colour_tex(1, 1, 2)], ids=["flat64", "1x1"])
def test_all_zero_maps_write_the_zero_map_file(oracle, img):
    fitted = oracle.encode(img, distance=1.0, side_info=dict(cfl="fitted"))
    ytox, ytob = U.maps_of(oracle.decode(fitted, want_dump=True))
    assert not ytox.any() and not ytob.any()
    assert fitted == oracle.encode(img, distance=1.0)
