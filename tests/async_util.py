"""The case table of the asynchronous-pipeline tests (tests/test_gpu_async_pipeline.py) and what the oracle says about it
(tests/test_async_cases.py checks the preconditions on the CPU).

Seven batches of 1, 3, 2, 5, 1, 4, 2 files.  The decoder has three workspace slots, so batches 0, 3, 6 share slot 0, batches 1, 4 slot 1
and batches 2, 5 slot 2: a slot that comes round again holds a larger, and then a smaller, layout than before, of other kinds of
frames.  Every batch is another selection of the kinds below with seeds of its own, so no two outputs that could be mistaken for one
another (same index, same shape, neighbouring batches or the same slot) hold the same bytes.  Options are read at submit time: one
batch is decoded at 1:8, one with the vector row loops on half-filled wavefronts.
"""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

import downscale_util as DU
import layer_util as LU
import noise_util as NU
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth, synth16

SLOTS = 3                     # JxlHipDecoder::kSlots
NOISE_LUT = [120, 200, 300, 420, 520, 640, 760, 900]
LAYER_AT = (20, 15)           # where the second layer of the layered still lies on the canvas

# name -> (width, height) as coded
SIZES = {"lossy-rgba": (520, 300), "lossy-one-group": (200, 120), "lossless-rgb8": (300, 270), "lossless-rgba16": (264, 200),
         "lossy-noise": (300, 260), "oriented": (330, 270), "layered": (150, 110), "lossy-u16-pq": (200, 160)}

# (kinds of the batch's files, decoder options of the batch)
TABLE = [(["lossy-rgba"], {}),
         (["layered", "lossy-noise", "lossless-rgb8"], {}),
         (["lossy-rgba", "lossless-rgba16"], {"downscale": 8}),
         (["lossy-rgba", "lossy-u16-pq", "oriented", "lossless-rgb8", "lossy-one-group"], {}),
         (["layered"], {}),
         (["lossy-noise", "lossless-rgba16", "oriented", "lossy-one-group"], {"lane_stride": 2, "no_direct": 1}),
         (["lossy-rgba", "lossy-u16-pq"], {})]
DEFAULTS = {"downscale": 1, "lane_stride": 0, "no_direct": 0}


@dataclass
class Case:
    kind: str
    seed: int
    data: bytes
    shape: tuple                          # (h, w, c) of the full-size image as displayed
    dtype: type
    source: Optional[np.ndarray] = None   # lossless kinds: the pixels the file must decode to, as displayed
    oracle_ref: bool = False              # the oracle reads the file, and test_gpu_parity.check_pixels is the bar against it
    plain: Optional[bytes] = None         # lossy-noise: the same stream without the noise


@dataclass
class Batch:
    index: int
    cases: list
    options: dict = field(default_factory=dict)

    @property
    def files(self):
        return [c.data for c in self.cases]


def picture(w, h, seed, bits=8):
    """synth() with an alpha plane that depends on the seed as well (synth's own is a function of the size alone)."""
    img = synth(w, h, seed) if bits == 8 else synth16(w, h, seed)
    a = img[..., 3].astype(np.int64)
    span = 192 << (bits - 8)
    img[..., 3] = (64 << (bits - 8)) + (a - (64 << (bits - 8)) + 23 * seed * (1 << (bits - 8))) % span
    return img


def make_case(oracle, kind, seed):
    w, h = SIZES[kind]
    bare = dict(container=False)
    if kind == "lossy-rgba":
        img = picture(w, h, seed)
        return Case(kind, seed, oracle.encode(img, strategy_mode=2, seed=seed, **bare), img.shape, np.uint8, oracle_ref=True)
    if kind == "lossy-one-group":
        img = picture(w, h, seed)
        return Case(kind, seed, oracle.encode(img, distance=2.0, **bare), img.shape, np.uint8, oracle_ref=True)
    if kind == "lossless-rgb8":
        img = np.ascontiguousarray(picture(w, h, seed)[..., :3])
        return Case(kind, seed, oracle.encode(img, lossless=True, **bare), img.shape, np.uint8, source=img)
    if kind == "lossless-rgba16":
        img = picture(w, h, seed, 16)
        return Case(kind, seed, oracle.encode(img, lossless=True, bits=16, lossless_predictor=5, lossless_tree=1, **bare), img.shape,
                    np.uint16, source=img)
    if kind == "lossy-noise":
        img = np.ascontiguousarray(picture(w, h, seed)[..., :3])
        plain = oracle.encode(img, **bare)
        return Case(kind, seed, NU.noisy(plain, NOISE_LUT), img.shape, np.uint8, plain=plain)
    if kind == "oriented":
        img = picture(w, h, seed)
        return Case(kind, seed, oracle.encode(img, orientation=6, **bare), np.rot90(img, -1).shape, np.uint8, oracle_ref=True)
    if kind == "layered":
        kw = dict(lossless=True, **bare)
        full, small = picture(w, h, seed), picture(40, 30, seed + 1)
        canvas = oracle.encode(np.zeros_like(full), **kw)
        data = LU.layered(canvas, [LU.Layer(oracle.encode(full, **kw), crop=False), LU.Layer(oracle.encode(small, **kw), x0=LAYER_AT[0], y0=LAYER_AT[1])])
        want = full.copy()
        want[LAYER_AT[1]:LAYER_AT[1] + 30, LAYER_AT[0]:LAYER_AT[0] + 40] = small   # both layers replace
        return Case(kind, seed, data, full.shape, np.uint8, source=want)
    if kind == "lossy-u16-pq":
        img = picture(w, h, seed, 16)
        return Case(kind, seed, oracle.encode(img, colour=4, bits=16, **bare), img.shape, np.uint16)
    raise KeyError(kind)


_table = None


def table(oracle):
    """The seven batches, built once per process."""
    global _table
    if _table is None:
        _table = [Batch(b, [make_case(oracle, kind, 10 * b + 1 + k) for k, kind in enumerate(kinds)], dict(opts))
                  for b, (kinds, opts) in enumerate(TABLE)]
    return _table


def out_shape(case, options):
    """(h, w, c) of what the decoder writes for the case under the batch's options."""
    h, w, c = case.shape
    if options.get("downscale", 1) == 8:
        w, h = api.reduced_size(w, h, 8)
    return h, w, c


def frame_flags(h):
    """The frame flags of a layer_util.FrameHeader: a U64 behind frame_type (2 bits) and encoding (1 bit)."""
    bits = h.prefix[3:]
    sel = bits[0] | bits[1] << 1
    val = lambda n, at: sum(bits[at + k] << k for k in range(n))
    return {0: lambda: 0, 1: lambda: 1 + val(4, 2), 2: lambda: 17 + val(8, 2)}[sel]()


def expected(oracle, case, options):
    """What the oracle (and, where it cannot read the file, the rules in numpy) gives for the case under the batch's options; close
    to the GPU's output, and exactly it for the lossless kinds."""
    ds = options.get("downscale", 1) == 8
    if case.source is not None:
        return DU.box_mean_int(case.source) if ds else case.source
    if case.kind == "lossy-noise":
        assert not ds
        h, w, _ = case.shape
        return NU.reference_pixels(oracle.decode(case.plain, want_dump=True), w, h, NOISE_LUT)
    if not ds:
        return oracle.decode(case.data).pixels
    od = oracle.decode(case.data, want_dump=True)
    h, w, c = case.shape
    out = DU.reference_colour(od, case.dtype)
    if c == 4:
        out = np.concatenate([out, DU.box_mean_int(od.planes["alpha"].reshape(h, w).astype(case.dtype))[..., None]], axis=2)
    return out


def slot_mates(n=len(TABLE)):
    """Pairs of batches (a, b), a < b, that are neighbours in submission order or share a workspace slot."""
    return sorted({(a, b) for a in range(n) for b in range(a + 1, n) if b == a + 1 or (b - a) % SLOTS == 0})
