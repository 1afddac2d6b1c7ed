"""GPU tests of animation encode with a tolerance for "unchanged" (include/jxlfiletypeio.h, Part 6: jxlhip_encode_animation_changes;
DESIGN.md §2 "Animation encode", §4.14).

The tile maps of anim_tiles_tol_kernel are checked tile by tile against the numpy rule of encode_animation_tolerance_util applied to
the model's reference canvas, the rectangles against the model's, the files as the bit rule's are: decoded by this project's animation
decoder (lossless: every displayed image is the model's reference canvas, exactly, and within the tolerance of its frame) and - lossy -
displayed image by displayed image against the previous one with every rectangle replaced by the decode of its own file.  Canvases are
at most 150 x 70 (3 x 2 ragged tiles) and stacks at most 10 frames."""
import ctypes as C

import numpy as np
import pytest
import torch

import encode_animation_rects_util as RU
import encode_animation_tolerance_util as TU
import encode_animation_util as EU
from pdn_jpegxl_amd import api
from test_gpu_encode_animation import crop_of, item, random_frame

pytestmark = pytest.mark.gpu

W, H = 150, 70


@pytest.fixture(scope="module")
def encoder():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the product path has no CPU fallback")
    enc = api.Encoder(0)
    yield enc
    enc.close()


def same(a, b):
    """Equal in every bit (NaNs included)."""
    return a.shape == b.shape and a.dtype == b.dtype and bool((EU.bits_of(a) == EU.bits_of(b)).all())


# ---------------------------------------------------------------- 1. tolerance = 0 is today's file
def rects_entry(encoder, items, durations, lossless, max_rects, merge_pixels):
    """jxlhip_encode_animation_rects itself (api.Encoder.encode_animation goes through jxlhip_encode_animation_changes)."""
    n = len(items)
    px = (api.JxlHipPixels * n)()
    for i, it in enumerate(items):
        px[i] = api.JxlHipPixels(it.ptr, it.width, it.height, it.stride_bytes, it.channels, api._SAMPLE_TYPES[it.dtype], it.bits, api.KNOWN_PROFILE.index(it.colour))
    dur = (C.c_uint32 * n)(*durations)
    opt = api.EncoderOptions(1.0, 7, lossless)
    ao = api.AnimationOptions(100, 1, 0, 0, 0)
    ro = api.AnimationRectOptions(max_rects, merge_pixels)
    md = api.EncoderImageMetadata()
    err = api.ErrorInfo()
    L = encoder._L
    assert L.jxlhip_encode_animation_rects(encoder._h, n, px, dur, C.byref(opt), C.byref(ao), C.byref(ro), C.byref(md), C.byref(err)) == 0, err.errorMessage
    p, size = C.c_void_p(), C.c_size_t()
    assert L.jxlhip_encoder_result(encoder._h, 0, C.byref(p), C.byref(size))
    return C.string_at(p.value, size.value)


@pytest.mark.parametrize("lossless", [True, False], ids=["lossless", "lossy"])
@pytest.mark.parametrize("max_rects", [1, 4])
def test_tolerance_zero_is_the_file_without_it(encoder, lossless, max_rects):
    frames = TU.sprite_stack(n=5, noise=0)
    frames[3] = frames[2].copy()
    items = [item(f) for f in frames]
    durations = [1, 2, 3, 4, 5]
    old = rects_entry(encoder, items, durations, lossless, max_rects, 4096)
    parts = encoder.last_animation_frame_rects
    assert parts == RU.model_animation_frame_rects(frames, lossless, max_rects, 4096)
    assert encoder.encode_animation(items, durations, lossless=lossless, max_rects=max_rects) == old
    assert encoder.encode_animation(items, durations, lossless=lossless, max_rects=max_rects, tolerance=0.0) == old
    assert encoder.last_animation_frame_rects == parts
    if max_rects == 1:
        with pytest.raises(ValueError):
            encoder.last_animation_tiles(0)                           # the bit rule with one rectangle measures no tiles, as before


# ---------------------------------------------------------------- 2. the tile maps: every comparator, every chunk path
# tolerance; the largest move that is unchanged; the smallest that is changed - all exactly representable, no |a - b| near the tolerance
MOVES = {"uint8": (5.5, 5, 6), "uint16": (300.5, 300, 301), "float16": (0.0625, 0.0625, 0.0625 + 1.0 / 1024), "float32": (0.0625, 0.0625, 0.0625 + 1.0 / 1024)}


def base_frame(rng, w, h, nch, dtype):
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return rng.integers(64, 192, (h, w, nch)).astype(dtype)
    if dtype == np.uint16:
        return rng.integers(16384, 49152, (h, w, nch)).astype(dtype)
    return (rng.integers(512, 1536, (h, w, nch)) / 1024.0).astype(dtype)      # multiples of 1/1024 in [0.5, 1.5): exact in binary16


def moved(ref, places, c, delta):
    """ref with sample c of the pixels (x, y) moved by delta (exact in the frame's dtype)."""
    g = ref.copy()
    for x, y in places:
        v = g[y, x, c].astype(np.float64) + delta
        g[y, x, c] = v
        assert float(g[y, x, c]) == v
    return g


def places_of(w, h, pixel_bytes):
    """Where a kernel that walks rows in 16-byte chunks under 64 x 64 tiles can go wrong."""
    edges = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (0, h // 2), (w - 1, h // 2)]             # the first and last pixel of a row
    corners = [(x, y) for x in (63, 64, 127, 128) for y in (0, 63, 64, h - 1)]                        # the corners of the tiles
    row = w * pixel_bytes
    cut = row // 16 * 16                                                                             # the chunk the row's end cuts starts here
    first_in_cut = -(-cut // pixel_bytes)
    ragged = [(first_in_cut, 1), (first_in_cut - 1, 2), (first_in_cut + 1, 3)] if cut < row else []  # in it, astride its start, behind
    keep = []
    for x, y in edges + corners + ragged:
        if 0 <= x < w and 0 <= y < h and (x, y) not in keep:
            keep.append((x, y))
    return keep


def planted_frames(w, h, nch, dtype, lossless, max_rects):
    """Up to 10 frames, each made from the model's reference canvas as it stands by moving single samples exactly as far as is unchanged,
    or one step further; floats also through +0 / -0, NaNs and infinities.  Returns (frames, tolerance, the model after them)."""
    dtype = np.dtype(dtype)
    tol, at, past = MOVES[dtype.name]
    rng = np.random.default_rng(w * 100 + h * 10 + nch + dtype.itemsize)
    places = places_of(w, h, nch * dtype.itemsize)
    last = nch - 1                                                    # the last channel: alpha where there is one
    m = TU.Model([base_frame(rng, w, h, nch, dtype)], tol, lossless, max_rects, 0)
    frames = [m.shown[0]]

    def add(f):
        frames.append(f)
        m.add(f)

    add(moved(m.ref, places, 0, at))                                  # as far as is unchanged, everywhere: nothing is (R takes pixel (0, 0))
    assert m.parts[-1] == (1, 0, 0, 1, 1)
    add(moved(m.ref, places, 0, past))                                # one step further, everywhere
    add(moved(moved(m.ref, places[0::2], last, -past), places[1::2], last, -at))      # the last channel only, downwards, every other place
    add(moved(moved(m.ref, places[1::2], last, past), places[0::2], min(1, last), at))
    if dtype.kind == "f":
        u = np.uint16 if dtype.itemsize == 2 else np.uint32
        nan1, nan2, pinf, ninf, nzero = (0x7E01, 0x7E02, 0x7C00, 0xFC00, 0x8000) if dtype.itemsize == 2 else (0x7FC00001, 0x7FC00002, 0x7F800000, 0xFF800000, 0x80000000)
        spots = [p for p in [(w // 2, h // 2), (w - 2, 1), (1, h - 2), (w // 3, h - 1), (w - 1, h // 3), (w // 4, h // 4)] if p not in places]
        spots = [(x, y) for x, y in dict.fromkeys(spots) if 0 <= x < w and 0 <= y < h]
        # alpha is coded by its bits: NaNs and infinities go there; without alpha only the zeros are tried
        first = [0, nan1, pinf, nan1, ninf, None] if nch in (2, 4) else [0]
        then = [nzero, nan1, pinf, nan2, pinf, pinf] if nch in (2, 4) else [nzero]
        for patterns in (first, then):
            g = m.ref.copy()
            for (x, y), bits in zip(spots, patterns):
                if bits is not None:
                    EU.bits_of(g)[y, x, last] = u(bits)
            add(g)
    add(m.ref.copy())                                                 # R itself: nothing
    assert m.parts[-1][1:] == (0, 0, 1, 1)
    add(base_frame(rng, w, h, nch, dtype))                            # another picture
    assert len(frames) <= 10
    return frames, tol, m


KINDS = [(dt, nch) for dt in (np.uint8, np.uint16, np.float16, np.float32) for nch in (1, 2, 3, 4)]
CASES = [(W, H, dt, nch) for dt, nch in KINDS]
CASES += [(5, 3, np.uint8, 1), (3, 3, np.uint16, 2), (7, 2, np.float16, 1), (3, 2, np.float32, 1)]       # rows under 16 bytes, each comparator
CASES += [(16, 1, np.uint8, 1), (16, 1, np.uint16, 1), (16, 1, np.float16, 2), (17, 1, np.uint8, 1)]     # one chunk exactly; two; four; one and a byte
CASE_IDS = ["%dx%d-%s%sx%d" % (w, h, np.dtype(dt).kind, 8 * np.dtype(dt).itemsize, nch) for w, h, dt, nch in CASES]


@pytest.mark.parametrize("max_rects", [4, 1])
@pytest.mark.parametrize("w,h,dtype,nch", CASES, ids=CASE_IDS)
def test_tile_maps_and_rectangles_against_numpy(encoder, w, h, dtype, nch, max_rects):
    size = np.dtype(dtype).itemsize
    lossless = np.dtype(dtype).kind == "u"                            # (lossless floats are refused)
    frames, tol, model = planted_frames(w, h, nch, dtype, lossless, max_rects)
    # every frame a sample past a 16-byte boundary, rows further apart than they need be by another odd number of samples, and
    # other garbage between them
    items = [item(f, offset=size, pitch_extra=size * (1 + 2 * (k % 5)), seed=100 + k) for k, f in enumerate(frames)]
    assert all(it.ptr % 16 == size for it in items)
    encoder.encode_animation(items, 1, lossless=lossless, effort=1, max_rects=max_rects, merge_pixels=0, tolerance=tol)
    for p, want in enumerate(model.maps):
        got = encoder.last_animation_tiles(p)
        assert got.shape == want.shape and got.dtype == np.uint8
        assert (got == want).all(), (p, [(ty, tx, got[ty, tx].tolist(), want[ty, tx].tolist()) for ty, tx in zip(*np.nonzero((got != want).any(axis=2)))])
    with pytest.raises(ValueError):
        encoder.last_animation_tiles(len(frames) - 1)                 # n frames have n - 1 pairs
    assert encoder.last_animation_frame_rects == model.parts
    assert encoder.last_animation_rects == model.rects
    assert sum(1 for m in model.maps if (m != 255).any()) >= 4         # (the sequence did plant changes)


# ---------------------------------------------------------------- 3. against what is shown: not the predecessor, not per pixel
@pytest.mark.parametrize("max_rects", [1, 4])
def test_a_ramp_is_coded_every_fourth_frame(encoder, max_rects):
    base = random_frame(np.random.default_rng(1), W, H, 4, np.uint8) // 2
    frames = []
    for k in range(9):
        f = base.copy()
        f[20:30, 40:60] += k
        frames.append(f)
    encoder.encode_animation([item(f) for f in frames], 1, lossless=True, max_rects=max_rects, tolerance=3)
    region = (40, 20, 20, 10)
    assert encoder.last_animation_rects == [(0, 0, W, H)] + [region if k % 4 == 0 else (0, 0, 1, 1) for k in range(1, 9)]
    assert EU.model_rects(frames, True)[1:] == [region] * 8           # the bit rule codes every frame


@pytest.mark.parametrize("max_rects", [1, 4])
def test_the_reference_is_what_is_shown_inside_a_coded_box(encoder, max_rects):
    f0 = np.full((H, W, 1), 100, np.uint8)
    f1 = f0.copy()
    f1[10:13, 10:13] = 150                                            # the neighbours move by 50 ...
    f1[11, 11] = 104                                                  # ... the pixel by 4: unchanged, yet inside the box, so 104 is shown
    f2 = f1.copy()
    f2[11, 11] = 97                                                   # 7 from what is shown; 3 from frame 0, which a per-pixel reference would hold
    frames = [f0, f1, f2]
    file = encoder.encode_animation([item(f) for f in frames], 1, lossless=True, max_rects=max_rects, tolerance=4)
    assert encoder.last_animation_rects == [(0, 0, W, H), (10, 10, 3, 3), (11, 11, 1, 1)]
    assert encoder.last_animation_tiles(1)[0, 0].tolist() == [11, 11, 11, 11]
    with api.Animation(file) as a:
        got = a.read_all()
    assert got[1][11, 11, 0] == 104 and got[2][11, 11, 0] == 97


def test_an_unchanged_frame_still_moves_the_reference_at_its_one_pixel(encoder):
    f0 = np.full((H, W, 3), 100, np.uint8)
    frames = [f0]
    for v in (103, 107, 111, 116):                                    # pixel (0, 0), channel 1: +3, +4, +4 against what is shown, then +5
        f = f0.copy()
        f[0, 0, 1] = v
        frames.append(f)
    file = encoder.encode_animation([item(f) for f in frames], 1, lossless=True, tolerance=4)
    assert encoder.last_animation_rects == [(0, 0, W, H)] + [(0, 0, 1, 1)] * 4
    maps = [encoder.last_animation_tiles(p) for p in range(4)]
    assert all((m == 255).all() for m in maps[:3]) and maps[3][0, 0].tolist() == [0, 0, 0, 0]      # 107 and 111 are 7 and 11 from frame 0
    with api.Animation(file) as a:
        got = a.read_all()
    assert [int(g[0, 0, 1]) for g in got] == [100, 103, 107, 111, 116]


# ---------------------------------------------------------------- 4. end to end, lossless
def noisy_stack(dtype, nch, noise=3, n=8):
    """The sprite stack in another sample type: (frames, tolerance = twice the noise)."""
    scale = {"uint8": 1, "uint16": 200, "float16": 1.0 / 256, "float32": 1.0 / 256}[np.dtype(dtype).name]
    frames = [(f.astype(np.float64) * scale).astype(dtype) for f in TU.sprite_stack(n=n, nch=nch, noise=noise)]
    return frames, 2 * noise * scale


@pytest.mark.parametrize("dtype,nch", [(np.uint8, 4), (np.uint16, 1)], ids=["RGBA8", "Gray16"])
@pytest.mark.parametrize("max_rects", [1, 4])
def test_lossless_shows_the_reference_canvas_within_the_tolerance(encoder, dtype, nch, max_rects):
    frames, tol = noisy_stack(dtype, nch)
    durations = [3 + k for k in range(len(frames))]
    file = encoder.encode_animation([item(f) for f in frames], durations, lossless=True, max_rects=max_rects, tolerance=tol)
    model = TU.Model(frames, tol, True, max_rects, 4096)
    assert encoder.last_animation_frame_rects == model.parts
    with api.Animation(file) as a:
        got = a.read_all()
        assert a.info.num_displayed == len(frames) and a.info.num_codestream_frames == len(model.parts)
        assert [fr.duration for fr in a.frames] == durations
    for k in range(len(frames)):
        assert same(got[k], model.shown[k]), "displayed image %d" % k
    assert TU.worst_error(list(got), frames) <= tol
    assert any(not same(got[k], frames[k]) for k in range(1, len(frames)))                         # (it is not the bit rule's file)


# ---------------------------------------------------------------- 5. end to end, lossy
@pytest.mark.parametrize("dtype,nch", [(np.uint8, 3), (np.float16, 4)], ids=["RGB8", "RGBAf16"])
def test_lossy_display_is_the_rectangles_decoded_alone(encoder, dtype, nch):
    """Displayed image k = displayed image k - 1 with every rectangle of frame k replaced by the decode of that rectangle's own file,
    byte for byte - the identity of the bit rule's tests: the rectangles are coded from the caller's frame, whatever decided them."""
    frames, tol = noisy_stack(dtype, nch, n=6)
    kw = dict(distance=1.0, effort=1)
    file = encoder.encode_animation([item(f) for f in frames], 2, max_rects=4, tolerance=tol, **kw)
    parts = encoder.last_animation_frame_rects
    assert parts == TU.Model(frames, tol, False, 4, 4096).parts and len(parts) > len(frames)
    refs = [api.save_pixels(crop_of(frames[p[0]], p[1:]), **kw) for p in parts]
    if np.dtype(dtype) == np.uint8:
        EU.walk_frames(file, refs)                                    # (asserts each frame's bytes from its TOC on)
    with api.Animation(file) as a:
        got = a.read_all()
        assert a.info.num_displayed == len(frames)
    shown = None
    for k in range(len(frames)):
        shown = None if shown is None else shown.copy()
        for part, ref in zip(parts, refs):
            if part[0] != k:
                continue
            x, y, w, h = part[1:]
            alone = api.load_image(ref).pixels.reshape(h, w, nch)
            if shown is None:
                shown = alone.copy()
            shown[y:y + h, x:x + w] = alone
        assert same(got[k], shown), (k, int((EU.bits_of(got[k]) != EU.bits_of(shown)).sum()))


# ---------------------------------------------------------------- 6. noise
@pytest.mark.parametrize("lossless", [True, False], ids=["lossless", "lossy"])
def test_noise_within_the_tolerance_codes_what_the_clean_stack_codes(encoder, lossless):
    clean, noisy = TU.sprite_stack(noise=0), TU.sprite_stack(noise=3)
    clean_items, noisy_items = [item(f) for f in clean], [item(f) for f in noisy]
    for max_rects in (1, 4):
        encoder.encode_animation(clean_items, 1, lossless=lossless, effort=1, max_rects=max_rects)
        clean_parts, clean_rects = encoder.last_animation_frame_rects, encoder.last_animation_rects
        all_of_it = encoder.encode_animation(noisy_items, 1, lossless=lossless, effort=1, max_rects=max_rects)
        assert all(r[2] * r[3] > 0.9 * W * H for r in encoder.last_animation_rects)                # bits decide: every frame whole
        file = encoder.encode_animation(noisy_items, 1, lossless=lossless, effort=1, max_rects=max_rects, tolerance=6)
        assert encoder.last_animation_frame_rects == clean_parts and encoder.last_animation_rects == clean_rects
        assert len(file) < len(all_of_it), (len(file), len(all_of_it))
        if max_rects == 4:                                            # the sprite and the block in the far corner stay two rectangles
            assert [sum(1 for p in clean_parts if p[0] == k) for k in range(len(noisy))] == [1] + [2] * (len(noisy) - 1)


# ---------------------------------------------------------------- 7. structure
def test_key_frames_are_whole_and_reset_the_reference(encoder):
    frames, tol = noisy_stack(np.uint8, 4)
    items = [item(f) for f in frames]
    file = encoder.encode_animation(items, 1, lossless=True, key_interval=3, max_rects=4, tolerance=tol)
    model = TU.Model(frames, tol, True, 4, 4096, key_interval=3)
    assert encoder.last_animation_frame_rects == model.parts
    assert [r for k, r in enumerate(encoder.last_animation_rects) if k % 3 == 0] == [(0, 0, W, H)] * 3
    for p, want in enumerate(model.maps):                             # key frames are measured too; the frame behind one against it
        assert (encoder.last_animation_tiles(p) == want).all(), p
    with api.Animation(file) as a:
        got = a.read_all()
        assert a.entry_points == [0, 3, 6]
    for k in range(len(frames)):
        assert same(got[k], model.shown[k]), k
        if k % 3 == 0:
            assert same(got[k], frames[k])


@pytest.mark.parametrize("lossless", [True, False], ids=["lossless", "lossy"])
def test_the_bytes_do_not_depend_on_the_chunking(encoder, lossless):
    frames, tol = noisy_stack(np.uint8, 3, n=5)
    items = [item(f) for f in frames]
    kw = dict(lossless=lossless, effort=1, max_rects=4, tolerance=tol)
    file = encoder.encode_animation(items, 1, **kw)
    parts = encoder.last_animation_frame_rects
    assert encoder.encode_animation(items, 1, chunk_frames=1, **kw) == file
    assert encoder.last_animation_frame_rects == parts


def test_one_frame_two_frames_and_the_workspace_reused(encoder):
    frames, tol = noisy_stack(np.uint8, 4)
    one = encoder.encode_animation([item(frames[0])], 1, lossless=True, tolerance=tol)
    assert encoder.last_animation_rects == [(0, 0, W, H)] and encoder.last_animation_frame_rects == [(0, 0, 0, W, H)]
    with pytest.raises(ValueError):
        encoder.last_animation_tiles(0)
    assert one == encoder.encode_animation([item(frames[0])], 1, lossless=True)
    encoder.encode_animation([item(f) for f in frames[:2]], 1, lossless=True, tolerance=tol)
    model = TU.Model(frames[:2], tol, True)
    assert encoder.last_animation_rects == model.rects and (encoder.last_animation_tiles(0) == model.maps[0]).all()
    # another size and sample type on the same encoder, larger then smaller: the reference canvas and the table are laid out anew
    for w, h, dtype, nch in ((150, 70, np.float32, 4), (37, 29, np.uint16, 3), (150, 70, np.uint8, 4)):
        lossless = np.dtype(dtype).kind == "u"
        other, t, m = planted_frames(w, h, nch, dtype, lossless, 4)
        encoder.encode_animation([item(f) for f in other], 1, lossless=lossless, effort=1, max_rects=4, merge_pixels=0, tolerance=t)
        assert encoder.last_animation_frame_rects == m.parts
        assert all((encoder.last_animation_tiles(p) == want).all() for p, want in enumerate(m.maps))


def test_a_tolerance_beyond_the_range_codes_nothing(encoder):
    rng = np.random.default_rng(9)
    for dtype, tol in ((np.uint8, 255), (np.uint16, 1e9)):
        frames = [random_frame(rng, W, H, 3, dtype) for _ in range(4)]
        file = encoder.encode_animation([item(f) for f in frames], 1, lossless=True, max_rects=4, tolerance=tol)
        assert encoder.last_animation_rects == [(0, 0, W, H)] + [(0, 0, 1, 1)] * 3
        with api.Animation(file) as a:
            got = a.read_all()
        for k in range(1, 4):
            want = got[k - 1].copy()
            want[0, 0] = frames[k][0, 0]
            assert same(got[k], want)


def test_refusals_through_the_entry_and_the_encoder_stays_usable(encoder):
    frames, tol = noisy_stack(np.uint8, 4, n=3)
    items = [item(f) for f in frames]
    file = encoder.encode_animation(items, 1, lossless=True, tolerance=tol)
    for bad, message in ((-1.0, "the tolerance must not be negative"), (-1e-20, "the tolerance must not be negative"),
                         (float("nan"), "the tolerance must be a finite number"), (float("inf"), "the tolerance must be a finite number"),
                         (float("-inf"), "the tolerance must be a finite number")):
        with pytest.raises(api.JxlError) as e:
            encoder.encode_animation(items, 1, lossless=True, tolerance=bad)
        assert e.value.status == "EncodeError" and message in str(e.value), (message, str(e.value))
        assert encoder.last_animation_rects == [] and encoder.last_animation_frame_rects == []
        assert not encoder._L.jxlhip_encoder_result(encoder._h, 0, None, None)      # no result is left
        with pytest.raises(ValueError):
            encoder.last_animation_tiles(0)
    L = encoder._L                                                    # the options may not be NULL
    px = (api.JxlHipPixels * 1)()
    assert L.jxlhip_encode_animation_changes(encoder._h, 1, px, (C.c_uint32 * 1)(1), C.byref(api.EncoderOptions(1.0, 7, True)),
                                             C.byref(api.AnimationOptions(100, 1, 0, 0, 0)), C.byref(api.AnimationRectOptions(1, 0)), None, None,
                                             C.byref(api.ErrorInfo())) == api.ENCODER_STATUS.index("NullParameter")
    torch.cuda.synchronize()                                          # no device fault was left behind
    assert encoder.encode_animation(items, 1, lossless=True, tolerance=tol) == file
