"""Seeking in animations on the GPU (jxlhip_animation_seek / _entry_points / _position through api.Animation): every displayed image
fetched on its own, in several orders, against the references of the sequential tests - the numpy composite of test_gpu_layers, the
source pictures, the noise restatement - and never against the product's own sequential output."""
import ctypes as C

import numpy as np
import pytest

import animation_seek_util as SU
import animation_util as AU
import layer_util as LU
import noise_util as NU
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth
from test_animation_plan import H, W, mixed_frames
from test_gpu_animation import displayed_references
from test_gpu_layers import F, build
from test_gpu_noise import RAMP, check_u8

pytestmark = pytest.mark.gpu

SHUFFLE = [5, 0, 9, 2, 11, 7, 1, 10, 3, 8, 6, 4]   # fixed; orders of shorter files keep the entries below their length


def _px(rng, w, h, nch=4, bits=8):
    return rng.integers(0, 1 << bits, (h, w, nch), dtype=np.uint8 if bits <= 8 else np.uint16)


def _np(t, dtype):
    a = t.cpu().numpy()
    return a.view(np.uint16) if dtype == np.uint16 else a


def crops_frames():
    """The all-replace file of test_gpu_animation.test_all_replace_frames_with_crops_are_exact."""
    rng = np.random.default_rng(21)
    return [F(_px(rng, W, H), crop=False, duration=1, save=1), F(_px(rng, 30, 20), x0=-4, y0=30, duration=1, source=1, save=2),
            F(_px(rng, 30, 20), x0=50, y0=-5, duration=0, source=1), F(_px(rng, 11, 13), x0=20, y0=20, duration=2, source=2)]


def _files(oracle):
    """name -> (file, references, exact, frames or None)"""
    out = {}
    fr = mixed_frames()
    out["mixed8"] = (build(oracle, W, H, fr, animation=True), displayed_references(W, H, fr, 8, False), False, fr)
    fr = crops_frames()
    out["crops"] = (build(oracle, W, H, fr, animation=True), displayed_references(W, H, fr, 8, False), True, fr)
    fr = mixed_frames(16)
    out["premul16"] = (build(oracle, W, H, fr, bits=16, premul=True, animation=True), displayed_references(W, H, fr, 16, True), False, fr)
    fr = SU.keyed_frames()
    out["keyed"] = (build(oracle, SU.KW, SU.KH, fr, animation=True), displayed_references(SU.KW, SU.KH, fr, 8, False), False, fr)
    # the oracle's lossy animation (picture, then twice the picture turned by 180 degrees): every frame replaces every channel, so each
    # image is its frame's own decode - the reference test_oracle_lossy_animation_equals_the_single_frame_decodes uses
    img = synth(40, 30, 31)
    alone = [api.load_image(oracle.encode(p, distance=1.0)).pixels for p in (img, np.ascontiguousarray(img[::-1, ::-1]))]
    out["lossy"] = (oracle.encode(img, animation_frames=3, distance=1.0), [alone[0], alone[1], alone[1]], True, None)
    return out


@pytest.fixture(scope="module")
def files(oracle):
    return _files(oracle)


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
@pytest.mark.parametrize("name", ["mixed8", "crops", "premul16", "keyed", "lossy"])
def test_every_image_by_seek(files, name, order):
    data, refs, exact, frames = files[name]
    n = len(refs)
    js = {"ascending": list(range(n)), "descending": list(range(n))[::-1], "shuffled": [j for j in SHUFFLE if j < n]}[order]
    with api.Animation(data) as a:
        assert a.info.num_displayed == n
        entries = a.entry_points
        if frames is not None:
            assert entries == SU.model_entry_points(frames, a.info.width, a.info.height)
        for j in js:
            before = a.position
            a.seek(j)
            # where the decode resumes: the latest entry point, or where it stood
            e = max(x for x in entries if x <= j)
            first = a.frames[e].first_codestream_frame
            if j == before[1] or e <= sum(1 for f in a.frames if f.first_codestream_frame + f.num_codestream_frames <= before[0]) <= j:
                first = before[0]
            assert a.position == (first, j), (j, before)
            got = _np(a.next(1), a.dtype)
            assert got.shape[0] == 1
            AU.check_images(got[0], refs[j], exact)
            assert a.position == (a.frames[j].first_codestream_frame + a.frames[j].num_codestream_frames, j + 1)
        # frame(j), the end, and out of range
        AU.check_images(_np(a.frame(n - 1), a.dtype), refs[n - 1], exact)
        a.seek(n)
        assert a.next(1).shape[0] == 0
        for bad in (-1, n + 1):
            at = a.position
            with pytest.raises(ValueError):
                a.seek(bad)
            assert a.position == at
        a.rewind()
        assert a.position == (0, 0)
        AU.check_images(_np(a.next(1), a.dtype)[0], refs[0], exact)


def test_position_after_a_seek(files):
    data, refs, _, frames = files["keyed"]
    with api.Animation(data) as a:
        assert a.entry_points == SU.KEYED_ENTRY_POINTS
        ff = lambda j: SU.first_frame(frames, j)
        a.seek(7)
        assert a.position == (ff(4), 7)
        a.seek(5)                                  # back: the entry point again (the decode has not moved)
        assert a.position == (ff(4), 5)
        AU.check_images(a.next(1).cpu().numpy()[0], refs[5], False)
        assert a.position == (ff(6), 6)
        a.seek(7)                                  # forward, no entry point in (6, 7]: from where it stands
        assert a.position == (ff(6), 7)
        a.seek(11)                                 # across entry point 8
        assert a.position == (ff(8), 11)
        AU.check_images(a.next(1).cpu().numpy()[0], refs[11], False)
        a.seek(2)
        assert a.position == (0, 2)
        for cf in (1, 2):                          # cuts inside the gap do not show
            assert a.set_option("chunk_frames", cf) == 1
            a.seek(9)
            a.seek(7)
            AU.check_images(a.next(2).cpu().numpy()[1], refs[8], False)


@pytest.mark.parametrize("max_rects", [1, 4])
def test_encoder_key_frames_are_entry_points(max_rects):
    import torch
    from test_gpu_encode_animation import item
    rng = np.random.default_rng(70 + max_rects)
    w, h = 64, 48
    bg = _px(rng, w, h)
    frames = []
    for k in range(8):
        f = bg.copy()
        f[5 + 4 * k:9 + 4 * k, 3 + 7 * k:8 + 7 * k] = _px(rng, 5, 4)
        if max_rects > 1:
            f[40:44, 60 - 6 * k:64 - 6 * k] = _px(rng, 4, 4)     # a second block far from the first: several rectangles
        frames.append(f)
    assert torch.cuda.is_available()
    enc = api.Encoder(0)
    try:
        data = enc.encode_animation([item(f) for f in frames], 2, key_interval=3, lossless=True, max_rects=max_rects)
    finally:
        enc.close()
    with api.Animation(data) as a:
        assert a.info.num_displayed == 8
        assert a.entry_points == [0, 3, 6]
        a.seek(7)
        assert a.position == (a.frames[6].first_codestream_frame, 7)
        assert (a.next(1).cpu().numpy()[0] == frames[7]).all()
        for j in (4, 2, 5, 0, 3):
            assert (a.frame(j).cpu().numpy() == frames[j]).all(), j


def test_noise_seeds_hold_when_entering_mid_file(oracle):
    """The three-frame noise file of test_noise_uses_each_frames_own_seeds: image 2 entered directly is seeded with visible index 2."""
    w, h = 90, 70
    pics = [synth(w, h, 41 + k) for k in range(3)]
    plain = [oracle.encode(p, container=False) for p in pics]
    canvas = oracle.encode(pics[0], container=False, animation_frames=2)
    data = LU.layered(canvas, [LU.Layer(NU.with_noise(cs, RAMP), crop=False, flags=1, duration=10) for cs in plain])
    with api.Animation(data) as a:
        assert a.entry_points == [0, 1, 2]
        a.seek(2)
        assert a.position == (2, 2)
        got = a.next(1).cpu().numpy()[0]
    od = oracle.decode(plain[2], want_dump=True)
    ref = NU.reference_pixels(od, w, h, RAMP, seeds=(2, 0))
    assert (got[..., 3] == od.pixels[..., 3]).all()
    check_u8(got[..., :3], ref, "image 2 by seek")
    assert (ref != NU.reference_pixels(od, w, h, RAMP, seeds=(0, 0))).mean() > 0.05


def test_skipped_images_are_not_stored(files):
    """seek(j); next(1) takes a buffer of one image: placed inside a sentinel-filled allocation, nothing around it is touched."""
    import torch
    data, refs, _, _ = files["keyed"]
    with api.Animation(data) as a:
        nb = a.info.image_bytes
        for j, cf in ((7, 0), (3, 1), (11, 2)):
            assert a.set_option("chunk_frames", cf) == 1
            buf = torch.full((5 * nb,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            a.seek(j)
            n, err = C.c_int32(-1), api.ErrorInfo()
            st = a._L.jxlhip_animation_next(a._h, 1, buf.data_ptr() + 2 * nb, nb, C.byref(n), C.byref(err))
            assert st == 0 and n.value == 1, err.errorMessage
            host = buf.cpu().numpy()
            assert (host[:2 * nb] == 0xA5).all() and (host[3 * nb:] == 0xA5).all()
            AU.check_images(host[2 * nb:3 * nb].reshape(refs[j].shape), refs[j], False)
            assert a.position[1] == j + 1


def test_seek_in_front_of_a_damaged_frame_still_delivers(oracle):
    """Three whole frames, the last one damaged (as test_a_damaged_frame_is_named builds it): every image is an entry point; after the
    chunk of image 2 has failed, seeks to the images in front of it deliver them."""
    kw = dict(lossless=True, container=False, lossless_tree=1, lossless_predictor=5)
    pics = [synth(300, 280, 3), synth(300, 280, 5), synth(300, 280, 7)]
    files = [oracle.encode(p, **kw) for p in pics]
    canvas = oracle.encode(np.zeros((280, 300, 4), np.uint8), animation_frames=2, **kw)
    data = bytearray(LU.layered(canvas, [LU.Layer(f, crop=False, duration=1) for f in files]))
    mid = len(data) - (len(files[2]) - LU.read_image_header(files[2]).frame_start) // 2
    data[mid] ^= 0x55
    data[mid + 1] ^= 0xAA
    with api.Animation(bytes(data)) as a:
        assert a.entry_points == [0, 1, 2]
        a.seek(2)
        with pytest.raises(api.FormatError) as e:
            a.next(1)
        assert "animation, codestream frame 2: GPU decode failed" in str(e.value)
        assert a.position == (2, 2)
        a.seek(1)
        assert a.position == (1, 1)
        assert (a.next(1).cpu().numpy()[0] == pics[1]).all()
        a.seek(0)
        got = a.next(2).cpu().numpy()
        assert (got[0] == pics[0]).all() and (got[1] == pics[1]).all()
        with pytest.raises(api.FormatError):
            a.thumbnails(1)
        assert a.position == (2, 2)
