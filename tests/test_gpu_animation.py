"""Animations on the GPU: every displayed image of a file through api.Animation (jxlhip_animation_*), against the source pictures of
the oracle's own animations, LoadImage, and the numpy composite of test_gpu_layers for files that blend; and that the cuts between
chunks of frames do not show."""
import numpy as np
import pytest

import animation_util as AU
import layer_util as LU
import noise_util as NU
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth
from test_animation_plan import H, W, long_frames, mixed_frames, refused_files
from test_gpu_layers import F, build, composite
from test_gpu_noise import RAMP, check_u8

pytestmark = pytest.mark.gpu


def _px(rng, w, h, nch=4, bits=8):
    return rng.integers(0, 1 << bits, (h, w, nch), dtype=np.uint8 if bits <= 8 else np.uint16)


def read_all(data, **options):
    with api.Animation(data) as a:
        for k, v in options.items():
            assert a.set_option(k, v) == 1
        return a.read_all()


# ---------------------------------------------------------------- the oracle's animations
@pytest.mark.parametrize("w,h", [(1, 1), (9, 7), (257, 3), (300, 280)])
@pytest.mark.parametrize("kind", ["rgba8", "rgb16", "gray8"])
def test_oracle_lossless_animation(oracle, kind, w, h):
    rng = np.random.default_rng(w + h)
    nch, bits = {"rgba8": (4, 8), "rgb16": (3, 16), "gray8": (1, 8)}[kind]
    img = _px(rng, w, h, nch, bits)
    with api.Animation(oracle.encode(img, animation_frames=3, lossless=True, bits=bits)) as a:
        i = a.info
        assert (i.width, i.height, i.num_channels, i.bytes_per_sample, i.float_samples) == (w, h, nch, bits // 8, 0)
        assert (i.have_animation, i.tps_numerator, i.tps_denominator, i.num_loops, i.have_timecodes) == (1, 100, 1, 0, 0)
        assert i.num_displayed == 3 and i.num_codestream_frames == 3 and i.image_bytes == w * h * nch * bits // 8
        assert [f.duration for f in a.frames] == [10, 10, 10]
        assert [(f.first_codestream_frame, f.num_codestream_frames) for f in a.frames] == [(0, 1), (1, 1), (2, 1)]
        got = a.read_all()
    assert got.shape == (3, h, w, nch) and got.dtype == img.dtype
    assert (got[0] == img).all()
    assert (got[1] == img[::-1, ::-1]).all() and (got[2] == img[::-1, ::-1]).all()


@pytest.mark.parametrize("w,h", [(300, 280), (40, 30)])
def test_oracle_lossy_animation_equals_the_single_frame_decodes(oracle, w, h):
    """Every frame replaces every channel: the samples are each frame's own decode, so there is no tolerance."""
    img = synth(w, h, 31)
    got = read_all(oracle.encode(img, animation_frames=3, distance=1.0))
    alone = [api.load_image(oracle.encode(p, distance=1.0)).pixels for p in (img, np.ascontiguousarray(img[::-1, ::-1]))]
    assert got.shape == (3, h, w, 4)
    for k in range(3):
        assert (got[k] == alone[min(k, 1)]).all(), (k, int((got[k] != alone[min(k, 1)]).sum()))
    assert (got[0] != got[1]).any()


def test_noise_uses_each_frames_own_seeds(oracle):
    """Three displayed lossy frames with noise: frame k is seeded with visible index k, and compared with the numpy
    restatement under the tolerance of tests/test_gpu_noise.py."""
    w, h = 90, 70
    pics = [synth(w, h, 41 + k) for k in range(3)]
    plain = [oracle.encode(p, container=False) for p in pics]
    canvas = oracle.encode(pics[0], container=False, animation_frames=2)
    data = LU.layered(canvas, [LU.Layer(NU.with_noise(cs, RAMP), crop=False, flags=1, duration=10) for cs in plain])
    got = read_all(data)
    assert got.shape == (3, h, w, 4)
    for k in range(3):
        od = oracle.decode(plain[k], want_dump=True)
        ref = NU.reference_pixels(od, w, h, RAMP, seeds=(k, 0))
        assert (got[k][..., 3] == od.pixels[..., 3]).all()
        check_u8(got[k][..., :3], ref, "frame %d" % k)
        if k:
            assert (ref != NU.reference_pixels(od, w, h, RAMP, seeds=(0, 0))).mean() > 0.05   # the seeds matter


# ---------------------------------------------------------------- image 0 is LoadImage's
def test_image_zero_is_load_image(oracle):
    rng = np.random.default_rng(11)
    frames = [F(_px(rng, 48, 40), crop=False), F(_px(rng, 20, 20), x0=5, y0=5, mode=2), F(_px(rng, 10, 30), x0=30, y0=3, mode=1, duration=7, name=b"shown")]
    later = F(_px(rng, 48, 40), crop=False, name=b"later")
    files = [(oracle.encode(_px(rng, 50, 33), lossless=True), 1), (oracle.encode(synth(70, 50, 3), distance=1.0), 1),
             (build(oracle, 48, 40, frames[:2]), 1), (build(oracle, 48, 40, frames, animation=True, extra_after=later), 2)]
    for data, n in files:
        with api.Animation(data) as a:
            assert a.info.num_displayed == n
            got = a.read_all()
            names = [f.name_bytes for f in a.frames]
        one = api.load_image(data)
        assert got.shape[0] == n and (got[0] == one.pixels).all()
        assert names[0].decode() == (one.layer_name or "")
    assert names == [b"shown", b"later"]


# ---------------------------------------------------------------- blending
def displayed_references(w, h, frames, bits, premul):
    return [composite(w, h, frames, bits, True, premul, displayed=k) for k, s in enumerate(AU.shows(frames)) if s >= 0]


@pytest.fixture(scope="module")
def mixed8(oracle):
    frames = mixed_frames()
    return frames, build(oracle, W, H, frames, animation=True), displayed_references(W, H, frames, 8, False)


@pytest.mark.parametrize("bits,premul", [(8, False), (8, True), (16, False), (16, True)])
def test_every_displayed_image_against_the_composite(oracle, bits, premul):
    frames = mixed_frames(bits)
    data = build(oracle, W, H, frames, bits=bits, premul=premul, animation=True)
    with api.Animation(data) as a:
        assert a.info.num_displayed == 3 and a.info.num_codestream_frames == 6
        assert [(f.duration, f.name_bytes, f.first_codestream_frame, f.num_codestream_frames) for f in a.frames] == \
               [(3, b"first", 0, 2), (5, b"second", 2, 3), (1, b"third", 5, 1)]
        got = a.read_all()
    refs = displayed_references(W, H, frames, bits, premul)
    assert got.shape == (3, H, W, 4) and got.dtype == refs[0].dtype
    for k in range(3):
        AU.check_images(got[k], refs[k], exact=False)
    assert (got[0] != got[1]).any() and (got[1] != got[2]).any()


def test_all_replace_frames_with_crops_are_exact(oracle):
    """Replace-only frames take the route of output-type samples; crops read the slot the frame names outside them."""
    rng = np.random.default_rng(21)
    frames = [F(_px(rng, W, H), crop=False, duration=1, save=1), F(_px(rng, 30, 20), x0=-4, y0=30, duration=1, source=1, save=2),
              F(_px(rng, 30, 20), x0=50, y0=-5, duration=0, source=1), F(_px(rng, 11, 13), x0=20, y0=20, duration=2, source=2)]
    got = read_all(build(oracle, W, H, frames, animation=True), chunk_frames=1)
    refs = displayed_references(W, H, frames, 8, False)
    assert got.shape[0] == 3
    for k in range(3):
        AU.check_images(got[k], refs[k], exact=True)


# ---------------------------------------------------------------- cuts do not show
def every_way(data, n):
    """The file's displayed images by every chunking, by single steps, and again after a rewind."""
    outs = [read_all(data, chunk_frames=c) for c in (1, 2, 3, 0)]
    with api.Animation(data) as a:
        steps = [a.next(1).cpu().numpy() for _ in range(n)]
        assert a.next(1).shape[0] == 0 and a.next(5).shape[0] == 0   # the end of the file
        outs.append(np.concatenate(steps).view(outs[0].dtype))
        a.rewind()
        assert a.set_option("chunk_frames", 2) == 1
        first = a.next(2).cpu().numpy().view(outs[0].dtype)
        rest = a.next(n).cpu().numpy().view(outs[0].dtype)
        outs.append(np.concatenate([first, rest]))
    return outs


def test_cuts_do_not_show_in_the_mixed_file(mixed8):
    frames, data, refs = mixed8
    outs = every_way(data, 3)
    for o in outs:
        assert o.shape == (3, H, W, 4) and (o == outs[0]).all()
    for k in range(3):
        AU.check_images(outs[0][k], refs[k], exact=False)


def test_cuts_do_not_show_in_seventy_frames(oracle):
    """Frame 2 is saved to slot 3 and frame 68 blends onto it: the slot crosses every cut between them, the 64-frame one included."""
    frames = long_frames()
    data = build(oracle, 9, 7, frames, animation=True)
    outs = every_way(data, 70)
    for o in outs:
        assert o.shape == (70, 7, 9, 4) and (o == outs[0]).all()
    refs = displayed_references(9, 7, frames, 8, False)
    for k in range(70):
        AU.check_images(outs[0][k], refs[k], exact=k != 68)
    assert (outs[0][68][0, 0] == frames[2].px[0, 0]).all() and (outs[0][68][0, 0] != frames[67].px[0, 0]).any()   # outside the crop: slot 3


def test_still_of_sixty_six_frames(oracle):
    """More frames than a layered still may hold: the animation path composes it in two chunks, the canvas crossing the cut in slot 0."""
    rng = np.random.default_rng(8)
    frames = [F(_px(rng, 9, 7), crop=False)] + [F(_px(rng, 3, 3), x0=k % 7, y0=k % 5, mode=1) for k in range(65)]
    got = read_all(build(oracle, 9, 7, frames))
    assert got.shape == (1, 7, 9, 4)
    AU.check_images(got[0], composite(9, 7, frames, 8, True, False), exact=True)


@pytest.mark.parametrize("nch,bits,mode", [(2, 8, 2), (3, 16, 0), (1, 8, 1), (3, 8, 1), (2, 16, 0)])
def test_slots_of_every_width_cross_every_cut(oracle, nch, bits, mode):
    """One, two and three channels, 8- and 16-bit samples, blended (f32 slots) and replace-only (bit patterns of the output type in the
    slots): a cut behind every frame against no cut, and against the composite."""
    rng = np.random.default_rng(10 * nch + bits + mode)
    frames = [F(_px(rng, W, H, nch, bits), crop=False, duration=1, save=1),
              F(_px(rng, 30, 20, nch, bits), x0=-4, y0=30, mode=mode, source=1, duration=1, save=2),
              F(_px(rng, 21, 33, nch, bits), x0=50, y0=-5, mode=mode, source=2, save=3),
              F(_px(rng, 11, 13, nch, bits), x0=20, y0=20, mode=mode, source=3, duration=2, save=1),
              F(_px(rng, 40, 9, nch, bits), x0=9, y0=2, mode=mode, source=1, duration=1)]
    data = build(oracle, W, H, frames, bits=bits, animation=True)
    assert [c["live_out"] for c in AU.plan(data, 1).chunks] == [2, 4, 8, 2, 0]
    whole, cut = read_all(data), read_all(data, chunk_frames=1)
    assert whole.shape == (4, H, W, nch) and (whole == cut).all()
    refs = [composite(W, H, frames, bits, nch in (2, 4), False, displayed=k) for k, s in enumerate(AU.shows(frames)) if s >= 0]
    for k in range(4):
        AU.check_images(cut[k], refs[k], exact=mode in (0, 1))


def test_a_failed_chunk_leaves_the_slots_as_they_were(oracle):
    """Slot 1 is alive across a chunk that fails: frame 0 is saved to it, frames 1 and 2 blend onto it and are saved to it, frame 3
    blends onto it, and frame 2's sections are damaged.  next(2) behind image 0 is the chunk of frames 1 and 2, which loads slot 1 and
    stores it (frame 3 still reads it): the call fails after its compose launch has stored the slot, built from the damaged frame.  The
    image in front of the damaged frame must still come out right afterwards, because a chunk stores its slots beside the ones it
    loaded.  (With one buffer for both this test fails: image 1 is then blended onto what the failed chunk left.)"""
    kw = dict(lossless=True, container=False, lossless_tree=1, lossless_predictor=5)
    rng = np.random.default_rng(33)
    w, h = 300, 280   # (the size at which tests/test_gpu_layers.py shows that damaged sections are noticed)
    blend = [LU.Blending(2, 0, False, 1), LU.Blending(2, 0, False, 1)]
    frames = [F(synth(w, h, 3), crop=False, duration=1, save=1), F(_px(rng, 40, 30), x0=5, y0=7, mode=2, source=1, duration=1, save=1),
              F(synth(w, h, 7), crop=False, mode=2, source=1, duration=1, save=1), F(_px(rng, 20, 20), x0=50, y0=50, mode=2, source=1, duration=1)]
    files = [oracle.encode(fr.px, **kw) for fr in frames]
    canvas = oracle.encode(np.zeros((h, w, 4), np.uint8), animation_frames=2, **kw)
    layers = [LU.Layer(f, x0=fr.x0, y0=fr.y0, crop=fr.crop, duration=1, save_ref=fr.save, blending=blend if fr.mode else None)
              for f, fr in zip(files, frames)]
    good = LU.layered(canvas, layers)
    end2 = len(LU.layered(canvas, layers[:3], last_is_last=False))
    assert good[:end2] == LU.layered(canvas, layers[:3], last_is_last=False)
    data = bytearray(good)
    mid = end2 - (len(files[2]) - LU.read_image_header(files[2]).frame_start) // 2
    data[mid] ^= 0x55
    data[mid + 1] ^= 0xAA
    want = read_all(good)
    AU.check_images(want[1], composite(w, h, frames, 8, True, False, displayed=1), exact=False)
    chunks = AU.plan(bytes(data), 0, (1, 2)).chunks
    assert [(c["first"], c["count"], c["live_in"], c["live_out"]) for c in chunks] == [(0, 1, 0, 2), (1, 2, 2, 2)]   # the failing chunk stores slot 1
    with api.Animation(bytes(data)) as a:
        assert (a.next(1).cpu().numpy()[0] == want[0]).all()
        with pytest.raises(api.FormatError) as e:
            a.next(2)                                  # frames 1 and 2 in one chunk, which stores slot 1 before it is known to have failed
        assert "animation, codestream frame 2: GPU decode failed" in str(e.value)
        assert (a.next(1).cpu().numpy()[0] == want[1]).all()   # image 1, from the slot as frame 0 left it
        with pytest.raises(api.FormatError):
            a.next(1)
        a.rewind()
        assert (a.next(2).cpu().numpy() == want[:2]).all()


def test_a_single_cmyk_frame(oracle):
    import icc_util
    rng = np.random.default_rng(14)
    data = oracle.encode(_px(rng, 20, 10, 5), lossless=True, icc=icc_util.cmyk_profile(), cmyk=True)
    with api.Animation(data) as a:
        assert (a.info.num_displayed, a.info.num_channels) == (1, 5)
        got = a.read_all()
    assert (got[0] == api.load_image(data).pixels).all()


# ---------------------------------------------------------------- orientation
@pytest.mark.parametrize("orientation", [5, 6, 7, 8])
def test_orientation_of_two_displayed_images(oracle, orientation):
    rng = np.random.default_rng(orientation)
    w, h = 37, 23
    frames = [F(_px(rng, w, h), crop=False, duration=2), F(_px(rng, 15, 9), x0=20, y0=-2, mode=2, duration=2)]
    kw = dict(lossless=True, container=False)
    canvas = oracle.encode(np.zeros((h, w, 4), np.uint8), orientation=orientation, animation_frames=2, **kw)
    layers = [LU.Layer(oracle.encode(fr.px, **kw), x0=fr.x0, y0=fr.y0, crop=fr.crop, duration=fr.duration,
                       blending=[LU.Blending(fr.mode, 0, False, 0), LU.Blending(fr.mode, 0, False, 0)]) for fr in frames]
    with api.Animation(LU.layered(canvas, layers)) as a:
        assert (a.info.width, a.info.height, a.info.num_displayed) == (h, w, 2)
        got = a.read_all()
    for k in range(2):
        ref = composite(w, h, frames, 8, True, False, displayed=k)
        # EXIF orientation as displayed (test_gpu_layers.test_orientation): 5 transpose, 6 rotate 90 cw, 7 transverse, 8 rotate 90 ccw
        o = {5: ref.transpose(1, 0, 2), 6: ref[::-1].transpose(1, 0, 2), 7: ref[::-1, ::-1].transpose(1, 0, 2), 8: ref[:, ::-1].transpose(1, 0, 2)}[orientation]
        AU.check_images(got[k], o, exact=False)


# ---------------------------------------------------------------- the interface
def test_header_fields_and_timecodes_through_the_interface(oracle):
    rng = np.random.default_rng(24)
    kw = dict(lossless=True, container=False)
    canvas = AU.with_animation_header(oracle.encode(np.zeros((7, 9, 4), np.uint8), animation_frames=2, **kw), 24, 1001, 300, True)
    pics = [_px(rng, 9, 7) for _ in range(3)]
    layers = [LU.Layer(oracle.encode(p, **kw), crop=False, duration=d) for p, d in zip(pics, (4, 0, 300))]
    with api.Animation(AU.frames_with_timecodes(canvas, layers, [0x01020304, 7, 0xFFFFFFFF])) as a:
        i = a.info
        assert (i.have_animation, i.tps_numerator, i.tps_denominator, i.num_loops, i.have_timecodes) == (1, 24, 1001, 300, 1)
        assert [(f.duration, f.timecode) for f in a.frames] == [(4, 0x01020304), (300, 0xFFFFFFFF)]
        got = a.read_all()
    assert (got[0] == pics[0]).all() and (got[1] == pics[2]).all()


def test_refusals_and_what_load_image_still_reads(oracle):
    for name, data, msg in refused_files(oracle):
        with pytest.raises(api.FormatError) as e:
            api.Animation(data)
        assert msg in str(e.value), (name, str(e.value))
        assert api.load_image(data).pixels.shape == (30, 40, 4), name


def test_options_capacity_and_the_end(mixed8):
    import ctypes as C
    import torch
    _, data, _ = mixed8
    with api.Animation(data) as a:
        for name in ("band_rows", "band_first_row", "downscale"):
            assert a.set_option(name, 8) == 0
        assert a.set_option("chunk_frames", -1) == 0 and a.set_option("no_such_option", 1) == 0 and a.set_option("debug_taps", 1) == 0
        assert a.set_option("lane_stride", 64) == 1 and a.set_option("lane_stride", 0) == 1
        buf = torch.zeros(2 * a.info.image_bytes, dtype=torch.uint8, device="cuda")
        n, err = C.c_int32(-1), api.ErrorInfo()
        st = a._L.jxlhip_animation_next(a._h, 3, buf.data_ptr(), buf.numel(), C.byref(n), C.byref(err))
        assert api.DECODER_STATUS[st] == "InvalidParameter" and n.value == 0 and b"3 displayed images need" in err.errorMessage
        assert a.next(3).shape[0] == 3    # the refused call consumed nothing
        assert a.next(1).shape[0] == 0


def test_a_damaged_frame_is_named(oracle):
    """The second frame's section bytes are damaged: the host parse passes, the GPU flags the frame, and the error names it; the image
    in front of it still decodes, and the position stays in front of the chunk that failed."""
    kw = dict(lossless=True, container=False, lossless_tree=1, lossless_predictor=5)
    pics = [synth(300, 280, 3), synth(300, 280, 7)]
    files = [oracle.encode(p, **kw) for p in pics]
    canvas = oracle.encode(np.zeros((280, 300, 4), np.uint8), animation_frames=2, **kw)
    data = bytearray(LU.layered(canvas, [LU.Layer(f, crop=False, duration=1) for f in files]))
    mid = len(data) - (len(files[1]) - LU.read_image_header(files[1]).frame_start) // 2
    data[mid] ^= 0x55
    data[mid + 1] ^= 0xAA
    with api.Animation(bytes(data)) as a:
        assert (a.next(1).cpu().numpy()[0] == pics[0]).all()
        for _ in range(2):
            with pytest.raises(api.FormatError) as e:
                a.next(1)
            assert "animation, codestream frame 1: GPU decode failed" in str(e.value)
