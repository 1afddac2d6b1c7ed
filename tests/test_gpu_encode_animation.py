"""GPU tests of animation encode (include/jxlfiletypeio.h, Part 6: jxlhip_encode_animation).

What changed between two frames is checked against numpy through the rectangles the encoder reports; the files are checked three
ways: decoded by this project's animation decoder (lossless: exact), walked frame by frame against jxlhip_save_pixels of each
rectangle (headers by the rules, bytes equal from the TOC on), and - lossy - displayed image by displayed image against the previous
one with the rectangle replaced by the decode of that rectangle's own file (no tolerance: every frame decodes and filters alone).
Frames are tiny: 1 x 1, 9 x 7, 257 x 3 (rows with an unaligned tail; two groups) and 300 x 280 (four ragged groups)."""
import numpy as np
import pytest
import torch

import animation_util as AU
import encode_animation_util as EU
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth
from save_pixels_util import channels

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (9, 7), (257, 3), (300, 280)]


@pytest.fixture(scope="module")
def encoder():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the product path has no CPU fallback")
    enc = api.Encoder(0)
    yield enc
    enc.close()


def item(px, offset=0, pitch_extra=0, seed=None):
    """px (h, w, c) in device memory as an EncodeItem: `offset` bytes into its allocation (which is 256-byte aligned), rows pitch_extra
    bytes further apart than they need be; seed: what the bytes outside the rows are filled with (None: zeros)."""
    h, w, c = px.shape
    row = w * c * px.dtype.itemsize
    pitch = row + pitch_extra
    n = offset + h * pitch
    host = np.zeros(n, np.uint8) if seed is None else np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    rows = np.ascontiguousarray(px).view(np.uint8).reshape(h, row)
    for y in range(h):
        host[offset + y * pitch:offset + y * pitch + row] = rows[y]
    dev = torch.from_numpy(host).cuda()
    return api.EncodeItem(dev.data_ptr() + offset, w, h, c, px.dtype, stride_bytes=pitch, keep=dev)


def random_frame(rng, w, h, nch, dtype):
    if np.dtype(dtype).kind == "u":
        return rng.integers(0, 1 << (8 * np.dtype(dtype).itemsize), (h, w, nch)).astype(dtype)
    return rng.random((h, w, nch), np.float32).astype(dtype)


def flipped(f, x, y, c, mask=1):
    g = f.copy()
    EU.bits_of(g)[y, x, c] ^= mask          # (bits_of is a view of a contiguous array)
    return g


def change_sequence(rng, w, h, nch, dtype):
    """Frames of which each differs from its predecessor in one stated way."""
    fr = [random_frame(rng, w, h, nch, dtype)]
    for x, y in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 2)):   # a single sample at each corner and at the centre
        fr.append(flipped(fr[-1], x, y, 0))
    fr.append(flipped(fr[-1], w - 1, h // 2, nch - 1))   # the last sample of a row: the unaligned tail
    fr.append(fr[-1].copy())                             # nothing
    g = fr[-1].copy()
    g_bits = EU.bits_of(g)
    g_bits ^= 1                                          # everything (floats: the last bit of the mantissa)
    fr.append(g)
    if nch in (2, 4):
        fr.append(flipped(fr[-1], w // 3, h // 3, nch - 1))   # alpha only
    if np.dtype(dtype) == np.uint16:
        fr.append(flipped(fr[-1], w // 4, h // 2, 1, 0x00A5))   # the low byte only
    if np.dtype(dtype).kind == "f":
        c = nch - 1 if nch in (2, 4) else 0
        g = fr[-1].copy()
        g[h // 2, w // 4, c] = 0.0
        fr.append(g)
        g = g.copy()
        g[h // 2, w // 4, c] = -0.0                      # -0.0 against +0.0: the values are equal, the bits are not
        fr.append(g)
        assert (fr[-1] == fr[-2]).all() and EU.changed_box(fr[-2], fr[-1]) is not None
    if np.dtype(dtype) == np.float16 and nch == 4:
        g = fr[-1].copy()
        EU.bits_of(g)[h // 3, w // 2, 3] = 0x7E01        # a NaN (in alpha, which is coded by its bits) ...
        fr.append(g)
        fr.append(g.copy())                              # ... and the same NaN again: nothing changed, though NaN != NaN
        assert EU.changed_box(fr[-2], fr[-1]) is None and not (fr[-1] == fr[-2]).all()
    return fr


KINDS = [(np.uint8, 1), (np.uint8, 2), (np.uint8, 3), (np.uint8, 4), (np.uint16, 3), (np.float16, 4), (np.float32, 3)]


@pytest.mark.parametrize("dtype,nch", KINDS, ids=["u8x1", "u8x2", "u8x3", "u8x4", "u16x3", "f16x4", "f32x3"])
@pytest.mark.parametrize("w,h", SIZES, ids=["1x1", "9x7", "257x3", "300x280"])
def test_extents_against_numpy(encoder, w, h, dtype, nch):
    rng = np.random.default_rng(w * 1000 + h * 10 + nch)
    frames = change_sequence(rng, w, h, nch, dtype)
    lossless = np.dtype(dtype).kind == "u"                  # (lossless floats are refused: their rectangles are the snapped ones)
    encoder.encode_animation([item(f) for f in frames], 1, lossless=lossless, effort=1)
    assert encoder.last_animation_rects == EU.model_rects(frames, lossless)


@pytest.mark.parametrize("dtype,nch", [(np.uint8, 3), (np.uint8, 4), (np.uint16, 3), (np.float32, 3)], ids=["u8x3", "u8x4", "u16x3", "f32x3"])
def test_extents_with_strides_offsets_and_garbage_in_the_padding(encoder, dtype, nch):
    """Every frame at another offset into its allocation (a sample or more: the two rows of a pair are aligned differently) and with
    another pitch (odd in samples: the alignment changes from row to row), the bytes between the rows random and different."""
    w, h = 257, 9
    size = np.dtype(dtype).itemsize
    rng = np.random.default_rng(nch * 10 + size)
    frames = change_sequence(rng, w, h, nch, dtype)
    items = [item(f, offset=size * (k * 7 % 23), pitch_extra=size * (1 + 2 * (k % 5)), seed=100 + k) for k, f in enumerate(frames)]
    lossless = np.dtype(dtype).kind == "u"
    encoder.encode_animation(items, 1, lossless=lossless, effort=1)
    assert encoder.last_animation_rects == EU.model_rects(frames, lossless)


# ---------------------------------------------------------------- files
def moving_block(bg, block, n, repeat_at, all_new_at, rng):
    """n frames: bg with `block` (5 x 4 where the canvas has room) moving; frame repeat_at repeats its predecessor, frame all_new_at
    changes every sample."""
    h, w = bg.shape[:2]
    bh, bw = min(4, h), min(5, w)
    out = []
    for k in range(n):
        if k == repeat_at:
            out.append(out[-1].copy())
            continue
        if k == all_new_at:
            out.append((EU.bits_of(out[-1]) ^ 1).view(bg.dtype))
            continue
        f = bg.copy()
        x, y = int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1))
        f[y:y + bh, x:x + bw] = block[:bh, :bw]
        out.append(f)
    return out


LOSSLESS_KINDS = [(np.uint8, 4), (np.uint16, 3), (np.uint8, 1)]


@pytest.mark.parametrize("dtype,nch", LOSSLESS_KINDS, ids=["RGBA8", "RGB16", "Gray8"])
@pytest.mark.parametrize("w,h", SIZES, ids=["1x1", "9x7", "257x3", "300x280"])
def test_lossless_round_trip(encoder, w, h, dtype, nch):
    rng = np.random.default_rng(w + h + nch)
    frames = moving_block(random_frame(rng, w, h, nch, dtype), random_frame(rng, 5, 4, nch, dtype), 6, 3, 4, rng)
    durations = [1, 255, 256, 7, 65536, 3]
    file = encoder.encode_animation([item(f) for f in frames], durations, tps=(1000, 1001), loops=3, lossless=True)
    with api.Animation(file) as a:
        got = a.read_all()
        i = a.info
        assert (i.have_animation, i.tps_numerator, i.tps_denominator, i.num_loops, i.have_timecodes) == (1, 1000, 1001, 3, 0)
        assert i.num_displayed == len(frames) and i.num_codestream_frames == len(frames)
        assert [fr.duration for fr in a.frames] == durations
    assert got.shape == (len(frames), h, w, nch) and got.dtype == dtype
    for k, f in enumerate(frames):
        assert (got[k] == f).all(), "displayed image %d" % k
    first = api.load_image(file).pixels
    assert (first.reshape(h, w, nch) == frames[0]).all()


def crop_of(f, r):
    x, y, w, h = r
    return np.ascontiguousarray(f[y:y + h, x:x + w])


class Case:
    """An animation, its file, and the single-frame file of every rectangle by save_pixels: computed once, never changed."""

    def __init__(self, encoder, frames, **kw):
        self.frames, self.kw = frames, kw
        self.durations = [2 + k for k in range(len(frames))]
        self.file = encoder.encode_animation([item(f) for f in frames], self.durations, **kw)
        self.rects = encoder.last_animation_rects
        self.refs = [api.save_pixels(crop_of(f, r), **kw) for f, r in zip(frames, self.rects)]


def natural_frames(nch, n=5):
    """A synthetic picture with a patch of another moving over it; frame 2 repeats frame 1, frame 3 is another picture."""
    W, H = 300, 280
    bg, other, patch = channels(synth(W, H, 31), nch), channels(synth(W, H, 32), nch), channels(synth(40, 30, 33), nch)
    out = []
    for k in range(n):
        if k == 2:
            out.append(out[-1].copy())
        elif k == 3:
            out.append(other.copy())
        else:
            f = (other if k > 3 else bg).copy()
            x, y = 13 + 61 * k, 200 - 47 * k
            f[y:y + 30, x:x + 40] = patch
            out.append(f)
    return out


LOSSY = [(1, 3), (1, 4), (7, 3), (7, 4)]


@pytest.fixture(scope="module")
def lossy_cases(encoder):
    return {(effort, nch): Case(encoder, natural_frames(nch), distance=1.0, effort=effort) for effort, nch in LOSSY}


@pytest.fixture(scope="module")
def lossless_cases(encoder):
    out = {}
    for dtype, nch in LOSSLESS_KINDS:
        rng = np.random.default_rng(nch)
        frames = moving_block(random_frame(rng, 300, 280, nch, dtype), random_frame(rng, 5, 4, nch, dtype), 5, 2, 3, rng)
        out[(np.dtype(dtype).name, nch)] = Case(encoder, frames, lossless=True)
    return out


def check_frame_by_frame(case, lossless):
    frames = case.frames
    H, W = frames[0].shape[:2]
    n = len(frames)
    assert case.rects == EU.model_rects(frames, lossless)
    info, headers = EU.walk_frames(case.file, case.refs)          # (asserts the bytes from each TOC on)
    assert info.have_animation and not info.have_timecodes and (info.xsize, info.ysize) == (W, H)
    for k, (h, r) in enumerate(zip(headers, case.rects)):
        full = r == (0, 0, W, H)
        assert h.crop == (None if full else r), k
        if not lossless and not full and r[2:] != (1, 1):
            assert r[0] % 8 == 0 and r[1] % 8 == 0 and ((r[0] + r[2]) % 8 == 0 or r[0] + r[2] == W) and ((r[1] + r[3]) % 8 == 0 or r[1] + r[3] == H)
        assert h.frame_type == 0 and h.encoding == (1 if lossless else 0)
        assert all(b.mode == 0 and b.source == (0 if full else 1) for b in h.blending) and len(h.blending) == 1 + info.nec
        assert h.duration == case.durations[k] and h.is_last == (k == n - 1)
        assert h.save_ref == (0 if k == n - 1 else 1) and h.save_before_ct is False and h.name == b""


@pytest.mark.parametrize("effort,nch", LOSSY, ids=["e1-rgb", "e1-rgba", "e7-rgb", "e7-rgba"])
def test_lossy_frames_are_save_pixels_of_their_rectangles(lossy_cases, effort, nch):
    check_frame_by_frame(lossy_cases[(effort, nch)], False)


@pytest.mark.parametrize("dtype,nch", LOSSLESS_KINDS, ids=["RGBA8", "RGB16", "Gray8"])
def test_lossless_frames_are_save_pixels_of_their_rectangles(lossless_cases, dtype, nch):
    check_frame_by_frame(lossless_cases[(np.dtype(dtype).name, nch)], True)


@pytest.mark.parametrize("effort,nch", LOSSY, ids=["e1-rgb", "e1-rgba", "e7-rgb", "e7-rgba"])
def test_lossy_display_is_the_rectangles_decoded_alone(lossy_cases, effort, nch):
    """Displayed image k = displayed image k - 1 with the rectangle replaced by the decode of the rectangle's own file, byte for byte
    (the reasoning of test_gpu_layers.test_lossy_replace_layers_equal_their_standalone_decodes)."""
    case = lossy_cases[(effort, nch)]
    with api.Animation(case.file) as a:
        got = a.read_all()
    shown = None
    for k, (r, ref) in enumerate(zip(case.rects, case.refs)):
        alone = api.load_image(ref).pixels
        x, y, w, h = r
        alone = alone.reshape(h, w, nch)
        shown = alone.copy() if shown is None else shown.copy()
        shown[y:y + h, x:x + w] = alone
        assert got[k].shape == shown.shape and (got[k] == shown).all(), (k, int((got[k] != shown).sum()))


def test_key_frames_are_whole_and_read_nothing(encoder):
    rng = np.random.default_rng(5)
    frames = moving_block(random_frame(rng, 40, 24, 3, np.uint8), random_frame(rng, 5, 4, 3, np.uint8), 8, 6, 99, rng)   # (frame 6 repeats 5)
    file = encoder.encode_animation([item(f) for f in frames], 4, key_interval=3, lossless=True)
    rects = encoder.last_animation_rects
    assert rects == EU.model_rects(frames, True, 3)
    assert [k for k, r in enumerate(rects) if r == (0, 0, 40, 24)] == [0, 3, 6]
    p = AU.plan(file)
    for k, fr in enumerate(p.frames):
        assert fr["show"] == k and fr["partial"] == (0 if k in (0, 3, 6) else 1)
        assert fr["reads"] == (0 if k in (0, 3, 6) else 1 << 1), (k, fr)      # a key frame reads no slot; the others slot 1
        assert fr["save"] == (1 if k < 7 else -1)
    with api.Animation(file) as a:
        assert (a.read_all() == np.stack(frames)).all()


@pytest.mark.parametrize("lossless", [True, False], ids=["lossless", "lossy"])
def test_an_unchanged_frame_is_one_pixel_and_still_displayed(encoder, lossless):
    f = channels(synth(64, 48, 3), 3)
    frames = [f, f.copy(), f.copy()]
    file = encoder.encode_animation([item(x) for x in frames], [5, 6, 7], lossless=lossless)
    assert encoder.last_animation_rects == [(0, 0, 64, 48), (0, 0, 1, 1), (0, 0, 1, 1)]
    with api.Animation(file) as a:
        got = a.read_all()
        assert a.info.num_displayed == 3 and [fr.duration for fr in a.frames] == [5, 6, 7]
    if lossless:
        assert (got == np.stack(frames)).all()
    else:   # the pixel at (0, 0) is replaced by its own encode; everything else is image 0
        assert (got[1][1:] == got[0][1:]).all() and (got[1][0, 1:] == got[0][0, 1:]).all() and (got[2][1:] == got[0][1:]).all()


@pytest.mark.parametrize("lossless", [True, False], ids=["lossless", "lossy"])
def test_the_bytes_do_not_depend_on_the_chunking(encoder, lossless_cases, lossy_cases, lossless):
    case = lossless_cases[("uint8", 4)] if lossless else lossy_cases[(7, 4)]
    assert len(case.frames) == 5
    items = [item(f) for f in case.frames]
    for chunk in (1, 2, 0):
        assert encoder.encode_animation(items, case.durations, chunk_frames=chunk, **case.kw) == case.file, chunk
        assert encoder.last_animation_rects == case.rects


def test_one_frame(encoder):
    f = channels(synth(33, 17, 4), 4)
    for lossless in (True, False):
        file = encoder.encode_animation(torch.from_numpy(f[None]).cuda(), [9], lossless=lossless)
        assert encoder.last_animation_rects == [(0, 0, 33, 17)]
        with api.Animation(file) as a:
            got = a.read_all()
            assert a.info.num_displayed == 1 and a.info.have_animation == 1 and a.frames[0].duration == 9
        assert got.shape == (1, 17, 33, 4)
        if lossless:
            assert (got[0] == f).all()


def test_exif_and_xmp_are_written_once_in_front_of_the_codestream(encoder):
    f = channels(synth(24, 16, 6), 3)
    exif, xmp = b"\0\0\0\0II*\0" + bytes(range(40)), b"<x:xmpmeta xmlns:x='adobe:ns:meta/'/>"
    file = encoder.encode_animation([item(f), item(flipped(f, 3, 3, 1))], 1, lossless=True, exif=exif, xmp=xmp)
    still = api.save_pixels(f, lossless=True, exif=exif, xmp=xmp)
    assert file[:file.index(b"jxlc") - 4] == still[:still.index(b"jxlc") - 4] and file.count(exif) == 1 and file.count(xmp) == 1
    size = int.from_bytes(file[file.index(b"jxlc") - 4:file.index(b"jxlc")], "big")
    assert size == len(file) - (file.index(b"jxlc") - 4)          # the jxlc box spans the rest of the file
    with api.Animation(file) as a:
        assert a.info.num_displayed == 2 and (a.read_all()[0] == f).all()


def test_the_encoder_serves_batches_before_and_after(encoder):
    px = [channels(synth(70, 50, 8), 4), channels(synth(9, 9, 9), 3)]
    batch = [item(p) for p in px]
    batch[1].lossless = True
    before = encoder.encode_batch(batch)
    assert before[0] == api.save_pixels(px[0]) and before[1] == api.save_pixels(px[1], lossless=True)
    frames = [px[0], flipped(px[0], 5, 5, 0)]
    file = encoder.encode_animation([item(f) for f in frames], 1, lossless=True)
    with pytest.raises(api.JxlError, match="size differs"):
        encoder.encode_animation([item(px[0]), item(px[1])], 1)
    assert encoder.encode_batch(batch) == before
    assert encoder.encode_animation([item(f) for f in frames], 1, lossless=True) == file


def test_refusals(encoder):
    a = channels(synth(16, 12, 1), 3)
    ok = item(a)
    cases = [
        ([ok, item(channels(synth(16, 13, 1), 3))], dict(), "frame 1: its size differs"),
        ([ok, item(a.astype(np.uint16))], dict(), "frame 1: its sample type differs"),
        ([ok, item(channels(synth(16, 12, 1), 4))], dict(), "frame 1: its number of channels differs"),
        ([ok, ok], dict(effort=8), "frame 0: efforts 8 and 9"),
        ([ok, ok], dict(durations=[1, 0]), "frame 1: a duration of 0"),
        ([], dict(durations=[]), "at least one frame"),
        ([item(a.astype(np.float32) / 255)] * 2, dict(lossless=True), "frame 0: lossless float"),
        ([ok, ok], dict(tps=(100, 0)), "denominator"),
    ]
    for frames, kw, message in cases:
        kw = dict(kw)
        durations = kw.pop("durations", 1)
        with pytest.raises(api.JxlError) as e:
            encoder.encode_animation(frames, durations, **kw)
        assert e.value.status == "EncodeError" and message in str(e.value), (message, str(e.value))
        assert encoder.last_animation_rects == []
    torch.cuda.synchronize()                                     # no device fault was left behind
    file = encoder.encode_animation([ok, ok], 1, lossless=True)  # and the encoder is usable
    with api.Animation(file) as an:
        assert (an.read_all() == np.stack([a, a])).all()
