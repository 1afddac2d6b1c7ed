"""float64 numpy twin of the distance map ("Distance map: rules of this project"; not Butteraugli) and of the figures
the closed loop of efforts 8 and 9 is judged by.  Constants as DESIGN.md states them."""
import numpy as np

import noise_util as NU

K = 1.0
A0 = 0.02
S = (8.0, 1.0, 0.5)          # the format's default LF steps 1/4096, 1/512, 1/256 relative to Y's
TARGET_PERCENTILE = 0.9
B5_TAPS = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0


def reflect(v, n):
    """The loop filters' ReflectIndex: mirrored with the edge sample repeated, the reflection repeated until the index is inside."""
    while v < 0 or v >= n:
        v = -v - 1 if v < 0 else 2 * n - 1 - v
    return v


def _blur_axis(a, axis):
    n = a.shape[axis]
    out = np.zeros_like(a)
    for k, wgt in zip(range(-2, 3), B5_TAPS):
        idx = [reflect(i + k, n) for i in range(n)]
        out += wgt * np.take(a, idx, axis=axis)
    return out


def b5(a):
    """Separable [1 4 6 4 1] / 16: along the rows first, then along the columns."""
    return _blur_axis(_blur_axis(np.asarray(a, np.float64), 1), 0)


def srgb8_to_xyb(rgb):
    """(h, w, 3) uint8 sRGB -> (3, h, w) float64 XYB planes: the inverse of noise_util.xyb_to_srgb."""
    v = np.asarray(rgb, np.float64) / 255.0
    lin = np.where(v <= 0.04045, v / 12.92, np.power((v + 0.055) / 1.055, 2.4))
    mix = np.tensordot(np.linalg.inv(NU.OPSIN_INV), np.moveaxis(lin, 2, 0), axes=(1, 0))
    g = np.cbrt(np.maximum(mix - NU.OPSIN_BIAS, 0.0)) + np.cbrt(NU.OPSIN_BIAS)
    return np.stack([0.5 * (g[0] - g[1]), 0.5 * (g[0] + g[1]), g[2]])


def mask(orig_y):
    oy = np.asarray(orig_y, np.float64)
    return 1.0 / (1.0 + b5(np.abs(oy - b5(oy))) / A0)


def pixel_values(orig, recon):
    """P of every pixel for (3, h, w) XYB planes of the original and of the reconstruction."""
    orig = np.asarray(orig, np.float64)
    recon = np.asarray(recon, np.float64)
    m2 = mask(orig[1]) ** 2
    p = np.zeros(orig.shape[1:])
    for c in range(3):
        e = recon[c] - orig[c]
        low = b5(b5(e))
        high = e - low
        p += S[c] ** 2 * (m2 * high ** 2 + low ** 2)
    return p


def cell_distances(orig, recon):
    """(ceil(h / 8), ceil(w / 8)) float64: T = K * mean(P^2)^(1/4) per 8 x 8 cell clipped to the frame."""
    p2 = pixel_values(orig, recon) ** 2
    h, w = p2.shape
    h8, w8 = (h + 7) // 8, (w + 7) // 8
    out = np.empty((h8, w8))
    for by in range(h8):
        for bx in range(w8):
            out[by, bx] = K * p2[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8].mean() ** 0.25
    return out


def distance_map(a_rgb, b_rgb):
    """Cell distances of two (h, w, 3+) uint8 sRGB pictures; a is the original."""
    return cell_distances(srgb8_to_xyb(np.asarray(a_rgb)[..., :3]), srgb8_to_xyb(np.asarray(b_rgb)[..., :3]))


def target_of(cells):
    """tau: the cell distance of rank floor(0.9 * (n - 1)) in ascending order (numpy's percentile 90, method 'lower')."""
    flat = np.sort(np.asarray(cells, np.float64).reshape(-1))
    return float(flat[int(np.floor(TARGET_PERCENTILE * (flat.size - 1)))])


def cells_over(cells, tau):
    return int((np.asarray(cells).reshape(-1) > tau).sum())
