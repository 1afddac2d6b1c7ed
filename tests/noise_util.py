"""Lossy frames with synthetic noise for the tests, and a numpy reference of the rules of DESIGN.md §2 ("Noise: rules restated, not
pinned").

A noise frame is an oracle VarDCT encode whose section 0 (LfGlobal, or the only section of a one-group frame) gets the ten parameter
bytes (eight 10-bit values, LSB first) in front of it, with that TOC entry rewritten; layer_util then sets frame flag 1.  The encoder
writes the default base colour correlations (kx = 0, kb = 1), which rule 4 uses.

The reference: the generator in uint64 arithmetic, the convolution and the addition in float64, and XYB -> output samples in float64.
"""
import numpy as np

import layer_util as LU

TOC = (LU.B(10), LU.B(14, 1024), LU.B(22, 17408), LU.B(30, 4211712))
GROUP = 256


def _cdiv(a, b):
    return (a + b - 1) // b


def lut_bytes(lut10):
    assert len(lut10) == 8 and all(0 <= v < 1024 for v in lut10)
    w = LU.BitWriter()
    for v in lut10:
        w.u(10, int(v))
    return w.tobytes()   # 80 bits: ten whole bytes, so the section's own bits keep their alignment


def with_noise(cs: bytes, lut10, num_passes=1, param_bytes=None) -> bytes:
    """The single-frame bare VarDCT codestream cs with the noise parameters in front of its section 0 (TOC rewritten).  The frame
    flag is set afterwards (noisy()).  param_bytes: other bytes in their place (truncation tests)."""
    info, h, end = LU.frame_of(cs)
    assert h.encoding == 0, "noise frames are VarDCT"
    r = LU.BitReader(cs, end)
    assert not r.b(), "permuted TOCs are not handled here"
    r.pos = (r.pos + 7) // 8 * 8
    ng = _cdiv(info.xsize, GROUP) * _cdiv(info.ysize, GROUP)
    nlf = _cdiv(info.xsize, 8 * GROUP) * _cdiv(info.ysize, 8 * GROUP)
    n = 1 if (ng == 1 and num_passes == 1) else 1 + nlf + 1 + ng * num_passes
    sizes = [r.u32(*TOC) for _ in range(n)]
    data = (r.pos + 7) // 8
    assert data + sum(sizes) == len(cs), (data, sizes, len(cs))
    s0 = (lut_bytes(lut10) if param_bytes is None else param_bytes) + cs[data:data + sizes[0]]
    w = LU.BitWriter()
    w.raw(LU._bits_of(cs, info.frame_start * 8, end))
    w.b(False)
    w.align()
    for s in [len(s0)] + sizes[1:]:
        w.u32(s, *TOC)
    w.align()
    return cs[:info.frame_start] + w.tobytes() + s0 + cs[data + sizes[0]:]


def noisy(cs: bytes, lut10, num_passes=1) -> bytes:
    """cs (a bare oracle VarDCT encode) as a file whose one frame carries the noise flag and the parameters lut10."""
    return LU.layered(cs, [LU.Layer(with_noise(cs, lut10, num_passes), crop=False, flags=1)])


# ---------------------------------------------------------------- rule 2: the generator
M64 = (1 << 64) - 1


def splitmix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def seed_state(a, b, c, d):
    """(s0[8], s1[8]) as Python integers."""
    s0 = [splitmix64(((((a << 32) + b) & M64) + 0x9E3779B97F4A7C15) & M64)]
    s1 = [splitmix64(((((c << 32) + d) & M64) + 0x9E3779B97F4A7C15) & M64)]
    for _ in range(7):
        s0.append(splitmix64(s0[-1]))
        s1.append(splitmix64(s1[-1]))
    return s0, s1


def batches(s0, s1, count):
    """`count` batches of 16 u32 values from the states s0, s1 (uint64 arrays of shape (..., 8), updated in place): (count, ..., 16)."""
    out = np.empty((count,) + s0.shape[:-1] + (16,), np.uint32)
    with np.errstate(over="ignore"):
        for k in range(count):
            t, u = s0.copy(), s1
            o = t + u
            s0[...] = u
            t ^= t << np.uint64(23)
            t ^= u ^ (t >> np.uint64(18)) ^ (u >> np.uint64(5))
            s1[...] = t
            out[k, ..., 0::2] = (o & np.uint64(0xFFFFFFFF)).astype(np.uint32)
            out[k, ..., 1::2] = (o >> np.uint64(32)).astype(np.uint32)
    return out


def to_float(v):
    return ((v >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32)


def group_planes(a, b, x0, y0, gw, gh):
    """The three gh x gw f32 planes of the group at (x0, y0) for frame indexes (a, b)."""
    s0, s1 = seed_state(a, b, x0, y0)
    nb = _cdiv(gw, 16)
    raw = batches(np.array(s0, np.uint64), np.array(s1, np.uint64), 3 * gh * nb)
    return to_float(raw.reshape(3, gh, nb * 16)[:, :, :gw])


def random_planes(w, h, a=0, b=0):
    """R_k: (3, h, w) float32, every group filled on its own (all groups advance together; each keeps its own number of steps)."""
    gs = [(x0, y0, min(GROUP, w - x0), min(GROUP, h - y0)) for y0 in range(0, h, GROUP) for x0 in range(0, w, GROUP)]
    states = [seed_state(a, b, x0, y0) for x0, y0, _, _ in gs]
    s0 = np.array([s[0] for s in states], np.uint64)
    s1 = np.array([s[1] for s in states], np.uint64)
    steps = [3 * gh * _cdiv(gw, 16) for _, _, gw, gh in gs]
    raw = batches(s0, s1, max(steps))   # (steps, groups, 16)
    out = np.empty((3, h, w), np.float32)
    for g, (x0, y0, gw, gh) in enumerate(gs):
        nb = _cdiv(gw, 16)
        out[:, y0:y0 + gh, x0:x0 + gw] = to_float(np.ascontiguousarray(raw[:steps[g], g]).reshape(3, gh, nb * 16)[:, :, :gw])
    return out


# ---------------------------------------------------------------- rules 3 and 4
def convolve(R):
    """N_k = 0.22 (0.16 sum_5x5 R_k - 4 R_k) in float64, the frame edge mirrored with the edge sample repeated."""
    R = R.astype(np.float64)
    P = np.pad(R, ((0, 0), (2, 2), (2, 2)), mode="symmetric")
    h, w = R.shape[1:]
    s = np.zeros_like(R)
    for dy in range(5):
        for dx in range(5):
            s += P[:, dy:dy + h, dx:dx + w]
    return 0.22 * (0.16 * s - 4.0 * R)


def strength(lut, v):
    s = np.maximum(0.0, 6.0 * v)
    i = np.minimum(np.floor(s), 6).astype(np.int64)
    t = np.minimum(s - i, 1.0)
    lut = np.asarray(lut, np.float64)
    return np.clip(lut[i] + (lut[i + 1] - lut[i]) * t, 0.0, 1.0)


def add_noise(xyb, N, lut10, kx=0.0, kb=1.0):
    """xyb: (3, h, w) filtered planes X, Y, B; N: convolve() of the random planes; returns the planes with the noise added (float64)."""
    lut = np.asarray(lut10, np.float64) / 1024.0
    X, Y, B = (xyb[c].astype(np.float64) for c in range(3))
    sr, sg = strength(lut, (Y + X) / 2), strength(lut, (Y - X) / 2)
    red = (N[0] / 128 + N[2] * 127 / 128) * sr
    green = (N[1] / 128 + N[2] * 127 / 128) * sg
    rg = red + green
    return np.stack([X + kx * rg + (red - green), Y + rg, B + kb * rg])


# ---------------------------------------------------------------- XYB -> output samples
OPSIN_INV = np.array([[11.031566901960783, -9.866943921568629, -0.16462299647058826],
                      [-3.254147380392157, 4.418770392156863, -0.16462299647058826],
                      [-3.6588512862745097, 2.7129230470588235, 1.9459282392156863]])
OPSIN_BIAS = -0.0037930732552754493


def xyb_to_srgb(xyb):
    """(3, h, w) XYB planes -> (h, w, 3) sRGB-encoded float64 samples (nominal range [0, 1], the curve sign-symmetric)."""
    X, Y, B = (np.asarray(xyb[c], np.float64) for c in range(3))
    cb = np.cbrt(OPSIN_BIAS)
    g = np.stack([Y + X - cb, Y - X - cb, B - cb])
    mix = g ** 3 + OPSIN_BIAS
    lin = np.tensordot(OPSIN_INV, mix, axes=(1, 0))
    a = np.abs(lin)
    enc = np.where(a <= 0.0031308, 12.92 * a, 1.055 * np.power(a, 1 / 2.4) - 0.055)
    return np.moveaxis(np.copysign(enc, lin), 0, 2)


def to_samples(rgb, dtype):
    """Encoded float samples -> the output type: integers scaled, clamped, rounded half up; floats converted."""
    if np.dtype(dtype).kind == "f":
        return rgb.astype(dtype)
    top = float(np.iinfo(dtype).max)
    return np.floor(np.clip(rgb * top, 0, top) + 0.5).astype(dtype)


def planes_of(od, w, h):
    """The oracle's xyb_filtered dump as (3, h, w) float32."""
    return np.stack([od.planes["xyb_filtered"][c].reshape(h, w) for c in range(3)])


def reference_pixels(od, w, h, lut10, dtype=np.uint8, seeds=(0, 0)):
    """The colour samples (h, w, 3) the rules give for the plain stream's oracle decode `od` (want_dump=True) with noise lut10."""
    N = convolve(random_planes(w, h, *seeds))
    return to_samples(xyb_to_srgb(add_noise(planes_of(od, w, h), N, lut10)), dtype)
