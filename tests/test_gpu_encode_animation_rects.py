"""GPU tests of animation encode with several rectangles per frame (include/jxlfiletypeio.h, Part 6: jxlhip_encode_animation_rects;
DESIGN.md §2 "Animation encode", §4.14).

The tile change map (anim_tiles_kernel) is checked against numpy tile by tile; the rectangles against the model of
encode_animation_rects_util applied to numpy's map; the files as those of one rectangle per frame are: decoded by this project's
animation decoder (lossless: exact), walked codestream frame by codestream frame against jxlhip_save_pixels of each rectangle, and -
lossy - displayed image by displayed image against the previous one with every rectangle replaced by the decode of its own file.
Frames are tiny: at most 300 x 280 (5 x 5 tiles, the last ragged)."""
import ctypes as C

import numpy as np
import pytest
import torch

import encode_animation_rects_util as RU
import encode_animation_util as EU
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth
from save_pixels_util import channels
from test_gpu_encode_animation import crop_of, flipped, item, random_frame

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def encoder():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the product path has no CPU fallback")
    enc = api.Encoder(0)
    yield enc
    enc.close()


# ---------------------------------------------------------------- the tile map
KINDS = [(np.uint8, 1), (np.uint8, 2), (np.uint8, 3), (np.uint8, 4), (np.uint16, 3), (np.uint16, 4), (np.float16, 4), (np.float32, 3), (np.float32, 4)]
KIND_IDS = ["u8x1", "u8x2", "u8x3", "u8x4", "u16x3", "u16x4", "f16x4", "f32x3", "f32x4"]     # pixels of 1, 2, 3, 4, 6, 8, 8, 12, 16 bytes
SIZES = [(1, 1), (65, 63), (130, 129), (257, 3), (300, 280)]
SIZE_IDS = ["1x1", "65x63", "130x129", "257x3", "300x280"]
NOT_16 = [1, 2, 3, 5, 6, 7, 9, 10, 11, 13, 14, 15]     # samples; times a sample size of 1, 2 or 4 bytes: never a multiple of 16 bytes


def tile_sequence(rng, w, h, nch, dtype):
    """Frames of which each differs from its predecessor in one stated way, at and around the tile boundaries."""
    fr = [random_frame(rng, w, h, nch, dtype)]
    xs = sorted({x for x in (0, 63, 64, 65, w - 1) if x < w})
    ys = sorted({y for y in (0, 63, 64, h - 1) if y < h})
    for y in ys:
        for x in xs:
            fr.append(flipped(fr[-1], x, y, 0))                       # one sample
    if w > 64:
        fr.append(flipped(flipped(fr[-1], 63, h // 2, nch - 1), 64, h // 2, 0))   # the neighbours either side of a tile boundary, together
    fr.append(flipped(fr[-1], w - 1, h // 2, nch - 1))                # the last sample of a row
    fr.append(fr[-1].copy())                                          # nothing
    g = fr[-1].copy()
    g_bits = EU.bits_of(g)
    g_bits ^= 1                                                       # every sample
    fr.append(g)
    if nch in (2, 4):
        fr.append(flipped(fr[-1], w // 3, h // 3, nch - 1))           # alpha only
    if np.dtype(dtype) == np.uint16:
        fr.append(flipped(fr[-1], w // 4, h // 2, 1, 0x00A5))         # the low byte only
    if np.dtype(dtype).kind == "f":
        c = nch - 1 if nch in (2, 4) else 0
        g = fr[-1].copy()
        g[h // 2, w // 4, c] = 0.0
        fr.append(g)
        g = g.copy()
        g[h // 2, w // 4, c] = -0.0                                   # the values are equal, the bits are not
        fr.append(g)
        assert (fr[-1] == fr[-2]).all() and EU.changed_box(fr[-2], fr[-1]) is not None
        if nch == 4:
            g = fr[-1].copy()
            EU.bits_of(g)[h // 3, w // 2, 3] = 0x7E01 if g.dtype.itemsize == 2 else 0x7FC00001   # a NaN (in alpha, coded by its bits) ...
            fr.append(g)
            fr.append(g.copy())                                       # ... and the same NaN again: nothing changed, though NaN != NaN
            assert EU.changed_box(fr[-2], fr[-1]) is None and not (fr[-1] == fr[-2]).all()
    return fr


_runs = {}


def tile_run(encoder, w, h, dtype, nch, scattered):
    """The sequence encoded once with max_rects = 3: (frames, lossless, items, the tile maps, last_animation_rects), kept for the tests
    that share it."""
    key = (w, h, np.dtype(dtype).name, nch, scattered)
    if key not in _runs:
        rng = np.random.default_rng(w * 1000 + h * 10 + nch)
        frames = tile_sequence(rng, w, h, nch, dtype)
        size = np.dtype(dtype).itemsize
        if scattered:   # every frame at another offset (whole samples, never a multiple of 16 bytes) and pitch (odd in samples), garbage between the rows
            items = [item(f, offset=size * NOT_16[k % len(NOT_16)], pitch_extra=size * (1 + 2 * (k % 5)), seed=100 + k) for k, f in enumerate(frames)]
            assert all(it.ptr % 16 for it in items)
        else:
            items = [item(f) for f in frames]
            assert all(it.ptr % 16 == 0 for it in items)
        lossless = np.dtype(dtype).kind == "u"                        # (lossless floats are refused)
        encoder.encode_animation(items, 1, lossless=lossless, effort=1, max_rects=3, merge_pixels=0)
        maps = [encoder.last_animation_tiles(p) for p in range(len(frames) - 1)]
        with pytest.raises(ValueError):
            encoder.last_animation_tiles(len(frames) - 1)             # n frames have n - 1 pairs
        _runs[key] = (frames, lossless, items, maps, encoder.last_animation_rects)
    return _runs[key]


@pytest.mark.parametrize("scattered", [False, True], ids=["tight", "scattered"])
@pytest.mark.parametrize("dtype,nch", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("w,h", SIZES, ids=SIZE_IDS)
def test_tile_map_against_numpy(encoder, w, h, dtype, nch, scattered):
    frames, _, _, maps, _ = tile_run(encoder, w, h, dtype, nch, scattered)
    for p, got in enumerate(maps):
        want = RU.tile_boxes(frames[p], frames[p + 1])
        assert got.shape == want.shape and got.dtype == np.uint8
        assert (got == want).all(), (p, [(ty, tx, got[ty, tx].tolist(), want[ty, tx].tolist()) for ty, tx in zip(*np.nonzero((got != want).any(axis=2)))])


@pytest.mark.parametrize("scattered", [False, True], ids=["tight", "scattered"])
@pytest.mark.parametrize("dtype,nch", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("w,h", SIZES, ids=SIZE_IDS)
def test_the_two_kernels_agree(encoder, w, h, dtype, nch, scattered):
    """The frame's overall box reduced from the tile map equals what anim_extents_kernel measures (and numpy)."""
    frames, lossless, items, _, by_tiles = tile_run(encoder, w, h, dtype, nch, scattered)
    encoder.encode_animation(items, 1, lossless=lossless, effort=1, max_rects=1, merge_pixels=0)
    assert encoder.last_animation_rects == by_tiles
    assert by_tiles == EU.model_rects(frames, lossless)
    assert encoder.last_animation_frame_rects == [(k,) + r for k, r in enumerate(by_tiles)]


# ---------------------------------------------------------------- the rectangles
W, H = 300, 280


def changed(f, *blocks):
    """f with the low bit of every sample of the blocks (x, y, width, height) flipped."""
    g = f.copy()
    bits = EU.bits_of(g)
    for x, y, w, h in blocks:
        bits[y:y + h, x:x + w] ^= 1
    return g


A, B, THIRD = (10, 10, 20, 12), (250, 240, 9, 9), (140, 70, 8, 8)   # tiles (0, 0); (3, 3) and (4, 3); (2, 1): none touches another
NEAR = [(20, 20, 10, 10), (150, 20, 10, 10)]      # tiles (0, 0) and (2, 0): one box is 140 x 10, 1200 pixels more than the two


def block_frames(base):
    f = [base]
    f.append(changed(f[-1], A, B))                # two far-apart blocks
    f.append(changed(f[-1], A, B, THIRD))         # and a third
    f.append(changed(f[-1], *NEAR))               # two blocks one tile apart
    f.append(f[-1].copy())                        # unchanged
    f.append(changed(f[-1], (0, 0, W, H)))        # all changed
    f.append(changed(f[-1], B, A))
    return f


@pytest.mark.parametrize("lossless", [True, False], ids=["lossless", "lossy"])
def test_rectangles_by_the_model(encoder, lossless):
    rng = np.random.default_rng(11)
    frames = block_frames(random_frame(rng, W, H, 4, np.uint8))
    items = [item(f) for f in frames]
    seen = {}
    for m, p, ki in ((4, 0, 0), (2, 0, 0), (4, 1199, 0), (4, 1200, 0), (2, 0, 3), (16, 0, 0)):
        if not lossless and p in (1199, 1200):
            continue                                                  # (the snapped boxes cost something else: below)
        encoder.encode_animation(items, 1, lossless=lossless, effort=1, key_interval=ki, max_rects=m, merge_pixels=p)
        got = encoder.last_animation_frame_rects
        assert got == RU.model_animation_frame_rects(frames, lossless, m, p, ki), (m, p, ki)
        assert encoder.last_animation_rects == EU.model_rects(frames, lossless, ki), (m, p, ki)
        seen[(m, p, ki)] = got
    count = lambda got, k: sum(1 for r in got if r[0] == k)
    got = seen[(4, 0, 0)]
    assert [count(got, k) for k in range(7)] == [1, 2, 3, 2, 1, 1, 2]
    assert [r for r in got if r[0] in (4, 5)] == [(4, 0, 0, 1, 1), (5, 0, 0, W, H)]
    assert [count(seen[(2, 0, 0)], k) for k in range(7)] == [1, 2, 2, 2, 1, 1, 2]          # the third block joins one of the two
    assert [count(seen[(2, 0, 3)], k) for k in range(7)] == [1, 2, 2, 1, 1, 1, 1]          # frames 3 and 6 are key frames
    if lossless:
        assert count(seen[(4, 1199, 0)], 3) == 2 and [r for r in seen[(4, 1200, 0)] if r[0] == 3] == [(3, 20, 20, 140, 10)]
    else:   # snapped: (16, 16, 16, 16) and (144, 16, 16, 16); one box is 144 x 16, 1792 pixels more
        for p, n in ((1791, 2), (1792, 1)):
            encoder.encode_animation(items, 1, lossless=False, effort=1, max_rects=4, merge_pixels=p)
            got = encoder.last_animation_frame_rects
            assert got == RU.model_animation_frame_rects(frames, False, 4, p) and count(got, 3) == n


# ---------------------------------------------------------------- files
class Case:
    """An animation with several rectangles per frame, its file, and the single-frame file of every rectangle by save_pixels: computed
    once, never changed."""

    def __init__(self, encoder, frames, max_rects, merge_pixels, **kw):
        self.frames, self.kw = frames, dict(kw, max_rects=max_rects, merge_pixels=merge_pixels)
        self.lossless = bool(kw.get("lossless"))
        self.durations = [2 + 3 * k for k in range(len(frames))]
        self.file = encoder.encode_animation([item(f) for f in frames], self.durations, **self.kw)
        self.parts = encoder.last_animation_frame_rects
        self.rects = encoder.last_animation_rects
        assert self.parts == RU.model_animation_frame_rects(frames, self.lossless, max_rects, merge_pixels)
        self.refs = [api.save_pixels(crop_of(frames[p[0]], p[1:]), **kw) for p in self.parts]


def natural_frames(nch):
    """A synthetic picture with two patches of others moving over it, far apart; frame 2 repeats frame 1, frame 3 is another picture."""
    bg, other = channels(synth(W, H, 31), nch), channels(synth(W, H, 32), nch)
    one, two = channels(synth(40, 30, 33), nch), channels(synth(12, 20, 34), nch)
    out = []
    for k in range(6):
        if k == 2:
            out.append(out[-1].copy())
        elif k == 3:
            out.append(other.copy())
        else:
            f = (other if k > 3 else bg).copy()
            x, y = 13 + 9 * k, 200 - 7 * k
            f[y:y + 30, x:x + 40] = one
            x, y = 270 - 5 * k, 11 + 10 * k
            f[y:y + 20, x:x + 12] = two
            out.append(f)
    return out


FILE_CASES = {"lossless-rgba8": (4, dict(lossless=True)), "lossy-e1-rgb": (3, dict(distance=1.0, effort=1)), "lossy-e7-rgba": (4, dict(distance=1.0, effort=7))}


@pytest.fixture(scope="module")
def cases(encoder):
    out = {}
    for name, (nch, kw) in FILE_CASES.items():
        if kw.get("lossless"):
            frames = block_frames(random_frame(np.random.default_rng(4), W, H, nch, np.uint8))
        else:
            frames = natural_frames(nch)
        out[name] = Case(encoder, frames, 3, 0, **kw)
        assert max(sum(1 for p in out[name].parts if p[0] == k) for k in range(len(frames))) >= 2, name
    return out


@pytest.mark.parametrize("dtype,nch", [(np.uint8, 4), (np.uint16, 3), (np.uint8, 1)], ids=["RGBA8", "RGB16", "Gray8"])
def test_lossless_round_trip(encoder, dtype, nch):
    frames = block_frames(random_frame(np.random.default_rng(nch), W, H, nch, dtype))
    n = len(frames)
    durations = [1, 255, 256, 7, 65536, 3, 9]
    file = encoder.encode_animation([item(f) for f in frames], durations, tps=(1000, 1001), loops=3, lossless=True, max_rects=4, merge_pixels=0)
    parts = encoder.last_animation_frame_rects
    assert parts == RU.model_animation_frame_rects(frames, True, 4, 0) and len(parts) > n
    with api.Animation(file) as a:
        got = a.read_all()
        i = a.info
        assert (i.have_animation, i.tps_numerator, i.tps_denominator, i.num_loops, i.have_timecodes) == (1, 1000, 1001, 3, 0)
        assert i.num_displayed == n and i.num_codestream_frames == len(parts)
        assert [fr.duration for fr in a.frames] == durations
        assert [fr.num_codestream_frames for fr in a.frames] == [sum(1 for p in parts if p[0] == k) for k in range(n)]
    assert got.shape == (n, H, W, nch) and got.dtype == dtype
    for k, f in enumerate(frames):
        assert (got[k] == f).all(), "displayed image %d" % k
    assert (api.load_image(file).pixels.reshape(H, W, nch) == frames[0]).all()


@pytest.mark.parametrize("name", list(FILE_CASES))
def test_frames_are_save_pixels_of_their_rectangles(cases, name):
    case = cases[name]
    total = len(case.parts)
    info, headers = EU.walk_frames(case.file, case.refs)          # (asserts the bytes from each TOC on)
    assert info.have_animation and not info.have_timecodes and (info.xsize, info.ysize) == (W, H)
    assert len(headers) == total > len(case.frames)
    for c, (h, part) in enumerate(zip(headers, case.parts)):
        k, r = part[0], part[1:]
        full = r == (0, 0, W, H)
        ends_frame = c == total - 1 or case.parts[c + 1][0] != k
        assert h.crop == (None if full else r), c
        if not case.lossless and not full and r[2:] != (1, 1):
            assert r[0] % 8 == 0 and r[1] % 8 == 0 and ((r[0] + r[2]) % 8 == 0 or r[0] + r[2] == W) and ((r[1] + r[3]) % 8 == 0 or r[1] + r[3] == H)
        assert h.frame_type == 0 and h.encoding == (1 if case.lossless else 0)
        assert all(b.mode == 0 and b.source == (0 if full else 1) for b in h.blending) and len(h.blending) == 1 + info.nec
        assert h.duration == (case.durations[k] if ends_frame else 0), c
        assert h.is_last == (c == total - 1) and h.save_ref == (0 if c == total - 1 else 1) and h.name == b""
    # the rectangles of a frame are disjoint and lie in the frame's reported box
    for k, box in enumerate(case.rects):
        mine = [p[1:] for p in case.parts if p[0] == k]
        for i, a in enumerate(mine):
            assert box[0] <= a[0] and box[1] <= a[1] and a[0] + a[2] <= box[0] + box[2] and a[1] + a[3] <= box[1] + box[3]
            for b in mine[i + 1:]:
                assert a[0] + a[2] <= b[0] or b[0] + b[2] <= a[0] or a[1] + a[3] <= b[1] or b[1] + b[3] <= a[1]


@pytest.mark.parametrize("name", ["lossy-e1-rgb", "lossy-e7-rgba"])
def test_lossy_display_is_the_rectangles_decoded_alone(cases, name):
    """Displayed image k = displayed image k - 1 with every rectangle of frame k replaced by the decode of that rectangle's own file,
    byte for byte: the rectangles are disjoint, and every frame decodes and filters alone."""
    case = cases[name]
    nch = case.frames[0].shape[2]
    with api.Animation(case.file) as a:
        got = a.read_all()
        assert a.info.num_displayed == len(case.frames) and [fr.duration for fr in a.frames] == case.durations
    shown = None
    for k in range(len(case.frames)):
        shown = None if shown is None else shown.copy()
        for part, ref in zip(case.parts, case.refs):
            if part[0] != k:
                continue
            x, y, w, h = part[1:]
            alone = api.load_image(ref).pixels.reshape(h, w, nch)
            if shown is None:
                shown = alone.copy()
            shown[y:y + h, x:x + w] = alone
        assert got[k].shape == shown.shape and (got[k] == shown).all(), (k, int((got[k] != shown).sum()))


@pytest.mark.parametrize("name", ["lossless-rgba8", "lossy-e7-rgba"])
def test_the_bytes_do_not_depend_on_the_chunking(encoder, cases, name):
    case = cases[name]
    items = [item(f) for f in case.frames]
    for chunk in (1, 2, 0):
        assert encoder.encode_animation(items, case.durations, chunk_frames=chunk, **case.kw) == case.file, chunk
        assert encoder.last_animation_frame_rects == case.parts


def old_entry(encoder, items, durations, lossless):
    """jxlhip_encode_animation itself (api.Encoder.encode_animation goes through jxlhip_encode_animation_rects)."""
    n = len(items)
    px = (api.JxlHipPixels * n)()
    for i, it in enumerate(items):
        px[i] = api.JxlHipPixels(it.ptr, it.width, it.height, it.stride_bytes, it.channels, api._SAMPLE_TYPES[it.dtype], it.bits, api.KNOWN_PROFILE.index(it.colour))
    dur = (C.c_uint32 * n)(*durations)
    opt = api.EncoderOptions(1.0, 7, lossless)
    ao = api.AnimationOptions(100, 1, 0, 0, 0)
    md = api.EncoderImageMetadata()
    err = api.ErrorInfo()
    L = encoder._L
    assert L.jxlhip_encode_animation(encoder._h, n, px, dur, C.byref(opt), C.byref(ao), C.byref(md), C.byref(err)) == 0, err.errorMessage
    p, size = C.c_void_p(), C.c_size_t()
    assert L.jxlhip_encoder_result(encoder._h, 0, C.byref(p), C.byref(size))
    return C.string_at(p.value, size.value)


@pytest.mark.parametrize("lossless", [True, False], ids=["lossless", "lossy"])
def test_one_rectangle_through_the_new_entry_is_encode_animation(encoder, lossless):
    frames = block_frames(channels(synth(W, H, 35), 4))
    items = [item(f) for f in frames]
    durations = list(range(1, len(frames) + 1))
    old = old_entry(encoder, items, durations, lossless)
    rects = encoder.last_animation_rects
    assert rects == EU.model_rects(frames, lossless)
    for p in (0, 4096):                                               # (merge_pixels plays no part)
        assert encoder.encode_animation(items, durations, lossless=lossless, max_rects=1, merge_pixels=p) == old
        assert encoder.last_animation_rects == rects and encoder.last_animation_frame_rects == [(k,) + r for k, r in enumerate(rects)]
        with pytest.raises(ValueError):
            encoder.last_animation_tiles(0)
    assert encoder.encode_animation(items, durations, lossless=lossless, max_rects=3, merge_pixels=0) != old


def test_the_point_of_it(encoder):
    """Noise does not compress: a frame costs its pixels.  With one rectangle per frame, frames 1 .. 4 are nearly the canvas each
    (a block near one corner, a pixel near the opposite one): five canvases.  With several they are 21 pixels each: one canvas."""
    rng = np.random.default_rng(77)
    frames = [random_frame(rng, W, H, 4, np.uint8)]
    for k in range(1, 5):
        frames.append(changed(frames[-1], (7 + k, 5 + 2 * k, 5, 4), (W - 3 - k, H - 2 - k, 1, 1)))
    items = [item(f) for f in frames]
    one = encoder.encode_animation(items, 1, lossless=True, max_rects=1, merge_pixels=4096)
    assert all(r[2] * r[3] > 0.85 * W * H for r in encoder.last_animation_rects)
    many = encoder.encode_animation(items, 1, lossless=True, max_rects=4, merge_pixels=4096)
    assert [p[0] for p in encoder.last_animation_frame_rects] == [0, 1, 1, 2, 2, 3, 3, 4, 4]
    assert len(many) < len(one) / 2, (len(many), len(one))
    for file in (one, many):
        with api.Animation(file) as a:
            assert a.info.num_displayed == 5 and (a.read_all() == np.stack(frames)).all()


def test_the_encoder_serves_batches_before_and_after_and_refuses_in_words(encoder):
    px = [channels(synth(70, 50, 8), 4), channels(synth(9, 9, 9), 3)]
    batch = [item(p) for p in px]
    batch[1].lossless = True
    before = encoder.encode_batch(batch)
    assert before[0] == api.save_pixels(px[0]) and before[1] == api.save_pixels(px[1], lossless=True)
    wide = channels(synth(200, 50, 8), 4)
    frames = [wide, changed(wide, (1, 1, 2, 2), (190, 40, 3, 3))]      # tiles (0, 0) and (2, 0)
    items = [item(f) for f in frames]
    file = encoder.encode_animation(items, 1, lossless=True, max_rects=2, merge_pixels=0)
    assert len(encoder.last_animation_frame_rects) == 3
    for kw, message in ((dict(max_rects=0), "max_rects) must be 1..16"), (dict(max_rects=17), "max_rects) must be 1..16"), (dict(max_rects=-1), "max_rects) must be 1..16"),
                        (dict(max_rects=2, merge_pixels=-1), "merge_pixels must not be negative")):
        kw.setdefault("merge_pixels", 0)
        with pytest.raises(api.JxlError) as e:
            encoder.encode_animation(items, 1, lossless=True, **kw)
        assert e.value.status == "EncodeError" and message in str(e.value), (message, str(e.value))
        assert encoder.last_animation_rects == [] and encoder.last_animation_frame_rects == []
        assert not encoder._L.jxlhip_encoder_result(encoder._h, 0, None, None)      # no result is left
        with pytest.raises(ValueError):
            encoder.last_animation_tiles(0)
    torch.cuda.synchronize()                                          # no device fault was left behind
    assert encoder.encode_batch(batch) == before
    assert encoder.encode_animation(items, 1, lossless=True, max_rects=2, merge_pixels=0) == file
    with api.Animation(file) as a:
        assert (a.read_all() == np.stack(frames)).all()
