"""Side information that the oracle's writer can vary (oracle/jxo_codec.h: SideInfo): the numpy restatement of its two formulas and
the knob values that the CPU tests (test_oracle_side_info.py) and the GPU tests (test_gpu_side_info.py) share."""
import numpy as np

M32 = 0xFFFFFFFF


def side_hash(seed, x, y, k):
    """u(seed, x, y, k) of the writer, modulo 2^32 (x, y: integer arrays or scalars)."""
    x = np.asarray(x, np.uint64)
    y = np.asarray(y, np.uint64)
    u = (np.uint64(seed) * np.uint64(0x9E3779B1) + x * np.uint64(0x85EBCA6B) + y * np.uint64(0xC2B2AE35) + np.uint64(k) * np.uint64(0x27D4EB2F)) & np.uint64(M32)
    u ^= u >> np.uint64(15)
    u = (u * np.uint64(0x2C1B3C6D)) & np.uint64(M32)
    u ^= u >> np.uint64(12)
    return u


def formula_cfl(seed, w, h):
    """(ytox, ytob) of a w x h frame as flat int8 arrays over its 64 x 64 tiles: (u & 255) - 128 with k = 0 / 1, then the pinned
    extremes - tile 0 holds (-128, 127), tile 1 (127, -128)."""
    wt, ht = (w + 63) // 64, (h + 63) // 64
    ty, tx = np.mgrid[0:ht, 0:wt]
    ytox = ((side_hash(seed, tx, ty, 0) & np.uint64(255)).astype(np.int32) - 128).ravel()
    ytob = ((side_hash(seed, tx, ty, 1) & np.uint64(255)).astype(np.int32) - 128).ravel()
    ytox[0], ytob[0] = -128, 127
    if ytox.size > 1:
        ytox[1], ytob[1] = 127, -128
    return ytox.astype(np.int8), ytob.astype(np.int8)


def formula_sharpness(seed, w, h):
    """Sharpness of a w x h frame as a flat uint8 array over its 8 x 8 cells: u & 7 with k = 2, then cell 0 holds 0 and cell 1 holds 7."""
    w8, h8 = (w + 7) // 8, (h + 7) // 8
    by, bx = np.mgrid[0:h8, 0:w8]
    s = (side_hash(seed, bx, by, 2) & np.uint64(7)).astype(np.uint8).ravel()
    s[0] = 0
    if s.size > 1:
        s[1] = 7
    return s


def check_formula_planes(od, w, h, seed, cfl=True, sharpness=True):
    """The oracle's dump (and with it, through compare_stages, the GPU's planes) against the restated formulas."""
    if cfl:
        ytox, ytob = formula_cfl(seed, w, h)
        assert np.array_equal(od.planes["ytox"], ytox) and np.array_equal(od.planes["ytob"], ytob)
    if sharpness:
        assert np.array_equal(od.planes["sharpness"], formula_sharpness(seed, w, h))


def psnr(a, b):
    mse = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    return 10 * np.log10(255.0 ** 2 / max(mse, 1e-12))


# ---------------------------------------------------------------- the knobs, one by one
# color_factor walks through the four branches of its U32: 84 (the default value, written explicitly), 256, 2..257 and 258...
CFL_PARAMS = {"cf84": (84, 0.0625, 0.875, 9, -14), "cf256": (256, -0.125, 1.25, -128, 127), "cf11": (11, 0.03125, 0.75, 3, -2),
              "cf1000": (1000, 0.05, 1.05, 127, -128)}
LF_FACTORS = (0.03, 0.2, 0.45)                     # defaults 1/32, 1/4, 1/2: no channel coarser; none of the three is an F16 number
GABORISH = ((0.09, 0.07), (0.14, 0.05), (0.05, 0.1))
SHARP_LUT = (0.5, 0.0, 1.25, 0.3, 1.0, 0.2, 0.9, 0.6)   # non-monotone, one entry 0 (no filtering there), one above 1
EPF_CHANNEL_SCALE = (30.0, 7.0, 2.2)
EPF_SIGMA = (0.6, 0.7, 5.1, 0.8)                   # quant_mul, pass-0 and pass-2 sigma scales, border_sad_mul
QUANT_BIASES = (0.8, 0.85, 0.9, 0.25)              # defaults about 0.945, 0.930, 0.950, 0.145

# Source-fidelity cases: knobs that the writer compensates, in settings that take no precision away by design, so the decode must stay
# as close to the source as the default stream's.  That rules out two kinds of setting, which the other tests
# still decode and compare: qm scales / LF factors that make a channel's steps coarser than the defaults, and custom base correlations
# with all-zero maps - a base that is off the image's own correlation by a little puts X's residual between half a step and one step
# wherever Y has a coefficient, the worst place for the writer's dead-zone quantiser (|v| < 0.6 -> 0).  Here the fitted maps take the
# base back out, as an encoder that chose such a base would.
COMPENSATED = {
    "cfl-fitted": dict(cfl="fitted"),
    "cfl-formula": dict(cfl="formula", seed=5),
    "cfl-params-cf84": dict(cfl="fitted", cfl_params=CFL_PARAMS["cf84"]),
    "cfl-params-cf256": dict(cfl="fitted", cfl_params=CFL_PARAMS["cf256"]),
    "cfl-params-cf11": dict(cfl="fitted", cfl_params=CFL_PARAMS["cf11"]),
    "cfl-params-cf1000": dict(cfl="fitted", cfl_params=CFL_PARAMS["cf1000"]),
    "lf-factors": dict(lf_factors=LF_FACTORS),
    "qm-7-2": dict(qm_scales=(7, 2)),
    "qm-3-7": dict(qm_scales=(3, 7)),
    "qm-5-5": dict(qm_scales=(5, 5)),
    "quant-biases": dict(quant_biases=QUANT_BIASES),
    "all-compensated": dict(cfl="fitted", cfl_params=CFL_PARAMS["cf256"], lf_factors=LF_FACTORS, qm_scales=(5, 5), quant_biases=QUANT_BIASES),
}
# the same knobs in the settings left out above, and the knobs of the loop filters (they change the picture by design)
OTHER = {
    "cfl-params-cf84-zero-maps": dict(cfl_params=CFL_PARAMS["cf84"]),
    "cfl-params-cf256-zero-maps": dict(cfl_params=CFL_PARAMS["cf256"]),
    "cfl-params-cf11-zero-maps": dict(cfl_params=CFL_PARAMS["cf11"]),
    "cfl-params-cf1000-zero-maps": dict(cfl_params=CFL_PARAMS["cf1000"]),
    "cfl-params+formula": dict(cfl="formula", seed=6, cfl_params=CFL_PARAMS["cf256"]),
    "qm-0-7": dict(qm_scales=(0, 7)),
    "qm-7-0": dict(qm_scales=(7, 0)),
    "sharp-formula": dict(sharpness="formula", seed=7),
    "sharp-0": dict(sharpness=0),
    "sharp-7": dict(sharpness=7),
    "gaborish": dict(gaborish_weights=GABORISH),
    "sharp-lut": dict(sharp_lut=SHARP_LUT, sharpness="formula", seed=8),
    "epf-channel-scale": dict(epf_channel_scale=EPF_CHANNEL_SCALE),
    "epf-sigma": dict(epf_sigma=EPF_SIGMA),
}
EVERYTHING = dict(cfl="formula", sharpness="formula", seed=9, cfl_params=CFL_PARAMS["cf11"], lf_factors=LF_FACTORS, qm_scales=(4, 1),
                  gaborish_weights=GABORISH, sharp_lut=SHARP_LUT, epf_channel_scale=EPF_CHANNEL_SCALE, epf_sigma=EPF_SIGMA,
                  quant_biases=QUANT_BIASES)
KNOBS = dict(COMPENSATED, **OTHER, everything=EVERYTHING)
