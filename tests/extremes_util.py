"""Pictures of the lossy extremes tests (test_encode_extremes_host.py, test_gpu_encode_extremes.py): what a lossy save meets at the ends
of its distance range (SetLossyParams accepts 0.05 to 25) and outside the smooth synth() pictures every other encode test feeds -
quantised HF values in the thousands, densely filled 64x64 varblocks, a group whose coefficients are nearly all non-zero, frames with
no HF at all, float samples far above 1.0.  Every picture comes from numpy.random.default_rng(seed) or a closed form."""
import functools

import numpy as np

DISTANCES = (0.05, 0.1, 25.0)
HOSTILE_W, HOSTILE_H = 72, 40      # partial cells on both edges (72 = 9 x 8: a partial 64-wide region; 40 = 5 x 8), one group
HOSTILE = ("noise", "bw-noise", "step8", "blue-yellow8", "red-cyan1", "black", "white", "red", "blue")
SINGLE_COLOUR = ("black", "white", "red", "blue")
OTHERS = ("dense64", "full-group")
FLOATS = ("hdr-noise", "hdr-step")
EIGHT_BIT = HOSTILE + OTHERS
# effort of a save -> the oracle encoder's strategy_mode with the same transform set (test_gpu_encode.py: EFFORTS)
MODE_OF_EFFORT = {3: 1, 5: 4, 7: 0}


def _two_colours(mask, a, b):
    out = np.empty(mask.shape + (3,), np.uint8)
    out[...] = np.asarray(a, np.uint8)
    out[mask] = np.asarray(b, np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def picture(name):
    """The picture `name` as (h, w, c): uint8 RGB (full-group: RGBA) or, for the hdr pictures, float32 RGB.  Read-only, shared."""
    w, h = HOSTILE_W, HOSTILE_H
    x = np.arange(w)[None, :] + np.zeros((h, 1), np.int64)
    y = np.arange(h)[:, None] + np.zeros((1, w), np.int64)
    if name == "noise":
        px = np.random.default_rng(101).integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif name == "bw-noise":
        px = np.repeat((np.random.default_rng(102).integers(0, 2, (h, w, 1)) * 255).astype(np.uint8), 3, axis=2)
    elif name == "step8":
        px = _two_colours(x % 8 >= 4, (0, 0, 0), (255, 255, 255))
    elif name == "blue-yellow8":
        px = _two_colours(x % 8 >= 4, (0, 0, 255), (255, 255, 0))
    elif name == "red-cyan1":
        px = _two_colours((x + y) % 2 == 1, (255, 0, 0), (0, 255, 255))
    elif name in SINGLE_COLOUR:
        px = _two_colours(x < 0, {"black": (0, 0, 0), "white": (255, 255, 255), "red": (255, 0, 0), "blue": (0, 0, 255)}[name], (0, 0, 0))
    elif name == "dense64":
        px = (100 + np.random.default_rng(103).integers(-1, 2, (136, 200, 3))).astype(np.uint8)
    elif name == "full-group":
        px = np.random.default_rng(104).integers(0, 256, (264, 264, 4), dtype=np.uint8)
    elif name == "hdr-noise":
        px = (np.random.default_rng(105).random((40, 40, 3), dtype=np.float32) * np.float32(64.0)).astype(np.float32)
    elif name == "hdr-step":
        px = np.zeros((40, 40, 3), np.float32)
        px[:, np.arange(40) % 8 >= 4] = 1000.0
    else:
        raise KeyError(name)
    px = np.ascontiguousarray(px)
    px.setflags(write=False)
    return px


def coded(px):
    """The channels SaveImage codes for the 8-bit picture px (its pixel-format analysis): one colour channel when r == g == b
    everywhere, alpha only when some pixel is not opaque.  What the oracle's encoder is given, so both code the same frame."""
    gray = bool((px[..., 0] == px[..., 1]).all() and (px[..., 1] == px[..., 2]).all())
    alpha = px.shape[2] == 4 and bool((px[..., 3] != 255).any())
    chans = ([0] if gray else [0, 1, 2]) + ([3] if alpha else [])
    return np.ascontiguousarray(px[..., chans])


def bgra_surface(px):
    """The BGRA8 surface of an RGB or RGBA uint8 picture (a missing alpha is opaque)."""
    h, w, c = px.shape
    out = np.full((h, w, 4), 255, np.uint8)
    out[..., 0], out[..., 1], out[..., 2] = px[..., 2], px[..., 1], px[..., 0]
    if c == 4:
        out[..., 3] = px[..., 3]
    return out


def psnr8(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def by_cell(plane, h8, w8):
    """A dumped qcoef plane (every varblock's coefficients in its own cells) as (cells, 64)."""
    return plane.reshape(h8, 8, w8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)


@functools.lru_cache(maxsize=None)
def oracle_stream(name, distance, mode):
    """oracle.encode of picture `name` (8-bit pictures: the channels SaveImage would code) - computed once, shared by the tests."""
    import oracle_lib
    px = picture(name)
    if px.dtype == np.float32:
        return oracle_lib.encode(px, distance=distance, strategy_mode=mode, float_samples=32)
    return oracle_lib.encode(coded(px), distance=distance, strategy_mode=mode)


@functools.lru_cache(maxsize=None)
def oracle_dump(name, distance, mode):
    """oracle.decode(oracle_stream(...), want_dump=True), computed once; treat as read-only."""
    import oracle_lib
    return oracle_lib.decode(oracle_stream(name, distance, mode), want_dump=True)
