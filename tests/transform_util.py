"""The inverse Modular transforms restated in numpy / Python integers from the format's definition (ISO/IEC 18181-1, Annex H: RCT,
Palette, Squeeze), the channel-list bookkeeping of a transform list, and the case table that tests/test_transform_chains.py (CPU:
the oracle against this file) and tests/test_gpu_transform_chains.py (GPU: the product against the source and the oracle) share.

A transform list is what oracle_lib.encode(transforms=...) takes: ("rct", begin_c, rct_type), ("palette", begin_c, num_c),
("squeeze", [(horizontal, in_place, begin_c, num_c), ...]) with [] for the default parameters."""
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import numpy as np

from pdn_jpegxl_amd.synth import synth, synth16

# rct_type = 7 * permutation + kind.  Positions (relative to begin_c) that the first, second and third decoded channel go to.
PERMUTATIONS = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (1, 0, 2), (2, 1, 0)]


def inverse_rct(a, b, c, rct_type):
    """The three coded channels (int64 arrays) -> the three channels before the transform, in channel-list order."""
    perm, kind = divmod(rct_type, 7)
    if kind == 6:                      # YCgCo
        tmp = a - (c >> 1)
        e = c + tmp
        f = tmp - (b >> 1)
        d = f + b
    else:
        d = a
        f = c + a if kind & 1 else c
        e = b + a if kind >> 1 == 1 else (b + ((a + f) >> 1) if kind >> 1 == 2 else b)
    out = [None, None, None]
    for v, pos in zip((d, e, f), PERMUTATIONS[perm]):
        out[pos] = v
    return out


def inverse_palette(palette, index):
    """palette: (num_c, nb_colors); index: (h, w) -> num_c channels.  Only stored colours (no delta entries, no implicit colours)."""
    assert index.size == 0 or (index.min() >= 0 and index.max() < palette.shape[1])
    return [palette[c][index] for c in range(palette.shape[0])]


def _idiv(a, b):
    """Integer division that truncates toward zero (the definition's Idiv)."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def tendency(a, b, c):
    if a >= b >= c:
        x = _idiv(4 * a - 3 * c - b + 6, 12)
        if x - (x & 1) > 2 * (a - b):
            x = 2 * (a - b) + 1
        if x + (x & 1) > 2 * (b - c):
            x = 2 * (b - c)
        return x
    if a <= b <= c:
        x = _idiv(4 * a - 3 * c - b - 6, 12)
        if x + (x & 1) < 2 * (a - b):
            x = 2 * (a - b) - 1
        if x - (x & 1) < 2 * (b - c):
            x = 2 * (b - c)
        return x
    return 0


def inverse_hsqueeze(avg, res):
    """avg: (h, w1), res: (h, w2) with w1 == w2 or w1 == w2 + 1 -> (h, w1 + w2)."""
    h, w1 = avg.shape
    w2 = res.shape[1]
    assert res.shape[0] == h and w1 - w2 in (0, 1), (avg.shape, res.shape)
    out = np.zeros((h, w1 + w2), np.int64)
    for y in range(h):
        for x in range(w2):
            a = int(avg[y, x])
            nxt = int(avg[y, x + 1]) if x + 1 < w1 else a
            left = int(out[y, 2 * x - 1]) if x > 0 else a
            diff = int(res[y, x]) + tendency(left, a, nxt)
            first = a + _idiv(diff, 2)
            out[y, 2 * x] = first
            out[y, 2 * x + 1] = first - diff
        if w1 > w2:
            out[y, 2 * w2] = avg[y, w2]
    return out


def inverse_vsqueeze(avg, res):
    """The same along y: the transposes through inverse_hsqueeze."""
    return np.ascontiguousarray(inverse_hsqueeze(np.ascontiguousarray(avg.T), np.ascontiguousarray(res.T)).T)


# ---------------------------------------------------------------- channel-list bookkeeping
def default_squeeze(sizes, nb_meta):
    """The parameters that an empty Squeeze list stands for, from the sizes [(w, h), ...] of the channel list at that point."""
    first = nb_meta
    count = len(sizes) - nb_meta
    w, h = sizes[first]
    out = []
    if count > 2 and sizes[first + 1] == (w, h):     # chroma (the second and third channel) first, residuals to the end of the list
        out += [(True, False, first + 1, 2), (False, False, first + 1, 2)]
    if h > w and h > 8:
        out.append((False, True, first, count))
        h = (h + 1) // 2
    while w > 8 or h > 8:
        if w > 8:
            out.append((True, True, first, count))
            w = (w + 1) // 2
        if h > 8:
            out.append((False, True, first, count))
            h = (h + 1) // 2
    return out


def channel_list(nchan, w, h, transforms, colours=()):
    """Walks the list forward over channel sizes only.  colours: the colour count of each palette entry, in order.  Returns
    (sizes of the coded channel list [(w, h), ...], number of meta channels, steps), the steps being the list with every Squeeze
    expanded into single steps: ("rct", begin_c, type), ("palette", begin_c, num_c), ("squeeze", horizontal, in_place, begin_c, num_c)."""
    sizes = [(w, h)] * nchan
    nb_meta = 0
    steps = []
    colours = list(colours)
    for t in transforms:
        if t[0] == "rct":
            assert t[1] + 3 <= len(sizes) and sizes[t[1]] == sizes[t[1] + 1] == sizes[t[1] + 2]
            steps.append(t)
        elif t[0] == "palette":
            _, begin_c, num_c = t
            assert begin_c >= nb_meta and begin_c + num_c <= len(sizes)
            # the num_c channels become one index channel in their place; the colours go to a meta channel at the front of the list
            sizes[begin_c:begin_c + num_c] = [sizes[begin_c]]
            sizes.insert(0, (colours.pop(0), num_c))
            nb_meta += 1
            steps.append(t)
        else:
            for hor, in_place, begin_c, num_c in (t[1] or default_squeeze(sizes, nb_meta)):
                assert begin_c >= nb_meta and begin_c + num_c <= len(sizes)
                residuals = []
                for c in range(begin_c, begin_c + num_c):
                    cw, ch = sizes[c]
                    if hor:
                        sizes[c] = ((cw + 1) // 2, ch)
                        residuals.append((cw - (cw + 1) // 2, ch))
                    else:
                        sizes[c] = (cw, (ch + 1) // 2)
                        residuals.append((cw, ch - (ch + 1) // 2))
                at = begin_c + num_c if in_place else len(sizes)     # residuals: right behind their averages, or at the end of the list
                sizes[at:at] = residuals
                steps.append(("squeeze", hor, in_place, begin_c, num_c))
    assert not colours
    return sizes, nb_meta, steps


def undo_transforms(coded, nchan, w, h, transforms):
    """coded: the coded channel list as (h, w) integer arrays -> the nchan channels of the picture (int64)."""
    ch = [np.asarray(c, np.int64) for c in coded]
    # (the colour counts are read off the meta channels here; the bookkeeping test states them itself)
    n_pal = sum(1 for t in transforms if t[0] == "palette")
    colours = [ch[n_pal - 1 - k].shape[1] for k in range(n_pal)]
    sizes, _, steps = channel_list(nchan, w, h, transforms, colours)
    assert [c.shape for c in ch] == [(sh, sw) for sw, sh in sizes]
    for s in reversed(steps):
        if s[0] == "rct":
            b = s[1]
            ch[b:b + 3] = inverse_rct(ch[b], ch[b + 1], ch[b + 2], s[2])
        elif s[0] == "palette":
            _, begin_c, num_c = s
            assert ch[0].shape[0] == num_c
            ch[begin_c + 1:begin_c + 2] = inverse_palette(ch[0], ch[begin_c + 1])
            del ch[0]
        else:
            _, hor, in_place, begin_c, num_c = s
            at = begin_c + num_c if in_place else len(ch) - num_c
            for k in range(num_c):
                ch[begin_c + k] = (inverse_hsqueeze if hor else inverse_vsqueeze)(ch[begin_c + k], ch[at + k])
            del ch[at:at + num_c]
    assert len(ch) == nchan and all(c.shape == (h, w) for c in ch)
    return ch


def route_of(transforms):
    """The rule by which the decoder picks how the inverses run: "inline" (inside the output kernel) for at most four transforms,
    none of them a Squeeze or a Palette; otherwise "launches" (one launch per inverse step)."""
    plain = all(t[0] == "rct" for t in transforms)
    return "inline" if plain and len(transforms) <= 4 else "launches"


# ---------------------------------------------------------------- pictures
def rgb8(w, h, seed):
    return np.ascontiguousarray(synth(w, h, seed)[..., :3])


def rgba8(w, h, seed):
    return synth(w, h, seed)


def rgb16(w, h, seed):
    return np.ascontiguousarray(synth16(w, h, seed)[..., :3])


def rgba16(w, h, seed):
    return synth16(w, h, seed)


def noise8(w, h, seed, nch=3):
    return np.random.default_rng(seed).integers(0, 256, (h, w, nch), dtype=np.uint8)


def noisy_rgba8(w, h, seed):
    """synth() with per-pixel noise on every channel (synth alone is flat at a few pixels across)."""
    img = synth(w, h, seed).astype(np.int32) + np.random.default_rng(seed).integers(-24, 25, (h, w, 4))
    return np.ascontiguousarray(np.clip(img, 0, 255).astype(np.uint8))


def blocks16(w, h, seed):
    """16-bit RGB, 4 x 4 blocks of 0 or 65535 per channel: the largest steps the sample range has, next to each other."""
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, 2, ((h + 3) // 4, (w + 3) // 4, 3)).astype(np.uint16) * 65535
    return np.ascontiguousarray(np.kron(cells, np.ones((4, 4, 1), np.uint16))[:h, :w])


def colours_of(n, seed, nch=3):
    """n distinct colours of nch channels, n <= 1536: channel 0 and channel 1 // 40 together name the colour."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    col = np.zeros((n, nch), np.uint8)
    col[:, 0] = (k * 97 + 13) & 255
    if nch > 1:
        col[:, 1] = (k >> 8) * 40 + rng.integers(0, 40, n)
    for c in range(2, nch):
        col[:, c] = rng.integers(0, 256, n)
    return col


def few_colours(w, h, n, seed, nch=3):
    """A picture of exactly n colours: every colour once, the remaining pixels drawn from them."""
    assert n <= w * h
    rng = np.random.default_rng(seed + 1000)
    idx = np.concatenate([np.arange(n), rng.integers(0, n, w * h - n)])
    rng.shuffle(idx)
    return np.ascontiguousarray(colours_of(n, seed, nch)[idx].reshape(h, w, nch))


def with_alpha_levels(img, n, seed):
    """img (RGBA) with its alpha replaced by exactly n levels."""
    h, w = img.shape[:2]
    out = img.copy()
    out[..., 3] = few_colours(w, h, n, seed, 1)[..., 0]
    return out


def cmyka8(w, h, seed):
    """C, M, Y, K, A as stored."""
    return np.ascontiguousarray(np.concatenate([synth(w, h, seed), noise8(w, h, seed, 1)], axis=2)[..., [0, 1, 2, 4, 3]])


# ---------------------------------------------------------------- the case table
@dataclass
class Case:
    name: str
    group: str                       # "a" .. "f" as in the GPU file
    picture: Callable[[], np.ndarray]
    transforms: list
    route: str                       # "inline" / "launches", stated; the CPU file holds it against route_of
    bits: int = 8
    colours: List[int] = field(default_factory=list)   # colour count of each palette entry, in order
    zero_size: bool = False          # the coded channel list holds a channel without samples
    cmyk: bool = False
    _src: Optional[np.ndarray] = None

    @property
    def src(self):
        if self._src is None:
            self._src = self.picture()
            self._src.setflags(write=False)
        return self._src

    def encode(self, oracle, transforms=None, **kw):
        t = self.transforms if transforms is None else transforms
        if self.cmyk:
            import icc_util
            kw.update(icc=icc_util.cmyk_profile(), cmyk=True)
        return oracle.encode(self.src, lossless=True, bits=self.bits, transforms=t, **kw)

    def expected(self):
        """What a decoder hands out: the source; CMYK inks leave inverted (0 = no ink), alpha as it is."""
        if not self.cmyk:
            return self.src
        out = self.src.copy()
        out[..., :4] = 255 - out[..., :4]
        return out


# the five-entry chain of group c; cut to four it is the last list that runs inline
CHAIN5 = [("rct", 0, 9), ("rct", 1, 24), ("rct", 0, 40), ("rct", 1, 6), ("rct", 0, 17)]
H, V = True, False


def _cases():
    out = []

    def add(name, group, picture, transforms, route, **kw):
        out.append(Case(name, group, picture, transforms, route, **kw))

    # a. every rct_type on 40 x 24 RGB: alone; before the default Squeeze; four of them before a Palette (negative palette entries)
    for t in range(42):
        add("rct%02d" % t, "a", lambda t=t: rgb8(40, 24, 200 + t), [("rct", 0, t)], "inline")
        add("rct%02d+squeeze" % t, "a", lambda t=t: rgb8(40, 24, 250 + t), [("rct", 0, t), ("squeeze", [])], "launches")
    for t in (6, 13, 23, 41):
        add("rct%02d+palette" % t, "a", lambda t=t: few_colours(40, 24, 64, 300 + t), [("rct", 0, t), ("palette", 0, 3)], "launches", colours=[64])
    # b. offsets and depths
    for t in (10, 34):
        add("rgba8-rct%d@1" % t, "b", lambda t=t: rgba8(40, 24, 310 + t), [("rct", 1, t)], "inline")
        add("rgba16-rct%d@1" % t, "b", lambda t=t: rgba16(40, 24, 320 + t), [("rct", 1, t)], "inline", bits=16)
    for t in (5, 6, 41):
        add("blocks16-rct%d" % t, "b", lambda t=t: blocks16(40, 24, 330 + t), [("rct", 0, t)], "inline", bits=16)
    add("cmyka-rct20@2", "b", lambda: cmyka8(40, 24, 340), [("rct", 2, 20)], "inline", cmyk=True)   # the register array's fifth entry
    # c. chains on RGBA
    add("chain2", "c", lambda: rgba8(40, 24, 350), CHAIN5[:2], "inline")
    add("chain4", "c", lambda: rgba8(40, 24, 351), CHAIN5[:4], "inline")
    add("chain5", "c", lambda: rgba8(40, 24, 351), CHAIN5, "launches")
    add("same-type-twice", "c", lambda: rgba8(40, 24, 352), [("rct", 0, 12), ("rct", 0, 12)], "inline")
    add("chain3+squeeze", "c", lambda: rgba8(40, 24, 353), CHAIN5[:3] + [("squeeze", [])], "launches")
    # d. explicit Squeeze lists; both sizes odd (one more average than residuals in both directions)
    for w, h, pic, n in ((33, 17, rgb8, 3), (9, 7, noisy_rgba8, 4)):
        s = "%dx%d-" % (w, h)
        p = lambda w=w, h=h, pic=pic: pic(w, h, 360 + w)
        add(s + "h-only", "d", p, [("squeeze", [(H, True, 0, n)])], "launches")
        add(s + "v-only", "d", p, [("squeeze", [(V, True, 0, n)])], "launches")
        add(s + "in-place", "d", p, [("squeeze", [(H, True, 0, n), (V, True, 0, n)])], "launches")
        add(s + "residuals-last", "d", p, [("squeeze", [(H, False, 0, n), (V, False, 0, n)])], "launches")
        add(s + "chroma-only", "d", p, [("rct", 0, 6), ("squeeze", [(H, False, 1, 2), (V, False, 1, 2), (H, True, 1, 2)])], "launches")
        add(s + "two-squeezes", "d", p, [("squeeze", [(H, True, 0, n)]), ("squeeze", [(V, True, 0, n), (H, True, 0, n)])], "launches")
        add(s + "rct-over-averages", "d", p, [("squeeze", [(H, True, 0, 3)]), ("rct", 0, 13)], "launches")
        add(s + "rct-over-residuals", "d", p, [("squeeze", [(H, True, 0, 3)]), ("rct", 3, 13)], "launches")
    add("33x17-explicit-then-default", "d", lambda: rgb8(33, 17, 370), [("squeeze", [(H, True, 0, 3)]), ("squeeze", [])], "launches")
    add("64x9-six-times-h", "d", lambda: rgb8(64, 9, 371), [("squeeze", [(H, True, 0, 3)] * 6)], "launches")
    add("5x3-to-nothing", "d", lambda: noise8(5, 3, 372), [("squeeze", [(H, True, 0, 3)] * 4 + [(V, True, 0, 3)] * 3)], "launches", zero_size=True)
    add("1x300-default", "d", lambda: rgb8(1, 300, 373), [("rct", 0, 6), ("squeeze", [])], "launches", zero_size=True)
    add("300x1-default", "d", lambda: rgb8(300, 1, 374), [("rct", 0, 6), ("squeeze", [])], "launches", zero_size=True)
    add("2x257-h", "d", lambda: rgb8(2, 257, 375), [("squeeze", [(H, True, 0, 3)])], "launches")
    # e. palettes
    add("alpha-palette+rct@1", "e", lambda: with_alpha_levels(rgba8(40, 24, 380), 5, 380), [("palette", 3, 1), ("rct", 1, 10)], "launches", colours=[5])
    add("rgb-palette-beside-alpha", "e", lambda: np.ascontiguousarray(np.concatenate([few_colours(40, 24, 40, 381), rgba8(40, 24, 381)[..., 3:]], axis=2)),
        [("palette", 0, 3)], "launches", colours=[40])
    two = lambda: with_alpha_levels(np.ascontiguousarray(np.concatenate([few_colours(40, 24, 30, 382), rgba8(40, 24, 382)[..., 3:]], axis=2)), 7, 382)
    add("two-palettes", "e", two, [("palette", 0, 3), ("palette", 2, 1)], "launches", colours=[30, 7])
    add("palette+index-squeeze", "e", lambda: few_colours(33, 17, 50, 383), [("palette", 0, 3), ("squeeze", [(H, True, 1, 1), (V, True, 1, 1)])], "launches",
        colours=[50])
    for n in (1, 255, 256, 257, 1279, 1280):     # around the selector edges of the header's colour-count field
        add("palette-%d-colours" % n, "e", lambda n=n: few_colours(40, 40, n, 390 + n), [("palette", 0, 3)], "launches", colours=[n])
    # f. what the downstream consumers decode (reduced size, layered files)
    add("rct23+explicit-squeeze", "f", lambda: rgba8(64, 48, 395), [("rct", 0, 23), ("squeeze", [(H, True, 0, 4), (V, True, 0, 4), (H, False, 0, 3)])], "launches")
    add("two-palettes-64x48", "f", lambda: with_alpha_levels(np.ascontiguousarray(np.concatenate([few_colours(64, 48, 90, 396), rgba8(64, 48, 396)[..., 3:]], axis=2)), 9, 396),
        [("palette", 0, 3), ("palette", 2, 1)], "launches", colours=[90, 9])
    return out


CASES = _cases()
MIN_CASES = {"inline": 53, "launches": 80}     # group a alone: 42 inline, 46 launches


def cases_of(group):
    return [c for c in CASES if c.group == group]


# g. refusals: (name, picture, transforms ending in a declared - unchecked - entry)
REFUSALS = [
    ("rct-type-42", lambda: rgb8(16, 8, 400), [("declare", 0, 0, 42)]),
    ("rct-type-73", lambda: rgb8(16, 8, 400), [("declare", 0, 0, 73)]),                       # the field's largest value
    ("rct-past-the-channels", lambda: rgba8(16, 8, 401), [("declare", 0, 2, 6)]),
    ("rct-over-different-sizes", lambda: rgb8(16, 8, 402), [("squeeze", [(H, True, 1, 2)]), ("declare", 0, 0, 6)]),
    ("palette-past-the-channels", lambda: rgb8(16, 8, 403), [("declare", 1, 2, 3, 16, 0, 0)]),
    ("squeeze-past-the-channels", lambda: rgb8(16, 8, 404), [("declare", 2, [(H, True, 2, 2)])]),
    ("squeeze-from-inside-the-meta-channels", lambda: few_colours(16, 8, 12, 405), [("palette", 0, 3), ("declare", 2, [(H, True, 0, 2)])]),
]
