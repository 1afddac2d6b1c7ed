"""Thumbnails of animations on the GPU (jxlhip_animation_next_reduced, api.Animation.thumbnails): every displayed image at 1:8, reduced
inside the compose pass.  The reference is the rule of DESIGN.md §2 - the mean over each 8 x 8 cell of the displayed image
(downscale_util.box_mean_int / box_mean_float) - applied to the references of the full-size tests: the numpy composite of
test_gpu_layers and the source pictures.  Every output buffer has the size of the full-size images and is filled with a sentinel, so
a store addressed by full-size geometry lands in owned memory and is caught."""
import ctypes as C

import numpy as np
import pytest

import animation_seek_util as SU
import animation_util as AU
import downscale_util as DU
import layer_util as LU
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth
from test_animation_plan import H, W, long_frames, mixed_frames
from test_gpu_layers import F, build, composite

pytestmark = pytest.mark.gpu


def _px(rng, w, h, nch=4, bits=8):
    return rng.integers(0, 1 << bits, (h, w, nch), dtype=np.uint8 if bits <= 8 else np.uint16)


def thumbs(a, count=0, step=1):
    """jxlhip_animation_next_reduced into a sentinel-filled buffer of the FULL size of the images asked for (count <= 0: all that are
    left).  Returns numpy [n, rh, rw, c]; every byte behind the n reduced images must still hold the sentinel."""
    import torch
    i = a.info
    left = -(-(i.num_displayed - a.position[1]) // step)
    want = left if count <= 0 else min(count, left)
    rw, rh = api.reduced_size(i.width, i.height, 8)
    each = rw * rh * i.num_channels * i.bytes_per_sample
    buf = torch.full((max(1, want) * i.image_bytes + 64,), DU.SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n, err = C.c_int32(-1), api.ErrorInfo()
    st = a._L.jxlhip_animation_next_reduced(a._h, want, step, buf.data_ptr(), buf.numel(), C.byref(n), C.byref(err))
    assert st == 0 and n.value == want, (st, n.value, want, err.errorMessage)
    host = buf.cpu().numpy()
    assert (host[want * each:] == DU.SENTINEL).all(), "bytes behind the reduced images were written (%d)" % int((host[want * each:] != DU.SENTINEL).sum())
    return host[:want * each].view(a.dtype).reshape(want, rh, rw, i.num_channels).copy()


def refs_of(w, h, frames, bits, has_alpha, premul=False):
    return [composite(w, h, frames, bits, has_alpha, premul, displayed=k) for k, s in enumerate(AU.shows(frames)) if s >= 0]


def replace_frames(rng, w, h, nch, bits):
    """Three displayed images, every frame replaces: the whole canvas, a crop that starts inside a cell and reaches past the canvas
    (outside it altogether on the smallest canvases), and one with negative offsets that ends inside a cell."""
    return [F(_px(rng, w, h, nch, bits), crop=False, duration=1, save=1),
            F(_px(rng, w // 2 + 3, h // 2 + 2, nch, bits), x0=3, y0=2, duration=1, source=1, save=1),
            F(_px(rng, (w + 1) // 2 + 2, (h + 1) // 2 + 1, nch, bits), x0=-2, y0=-1, duration=1, source=1)]


# ---------------------------------------------------------------- all-replace files: exact
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("nch", [1, 2, 3, 4])
@pytest.mark.parametrize("w,h", [(1, 1), (9, 7), (13, 70), (257, 3), (100, 60)])
def test_all_replace_files_are_exact(oracle, w, h, nch, bits):
    rng = np.random.default_rng(1000 * w + 10 * h + nch + bits)
    frames = replace_frames(rng, w, h, nch, bits)
    refs = refs_of(w, h, frames, bits, nch in (2, 4))
    with api.Animation(build(oracle, w, h, frames, bits=bits, animation=True)) as a:
        got = thumbs(a)
        assert a.position[1] == 3
        via_api = a.read_thumbnails()
    rw, rh = api.reduced_size(w, h, 8)
    assert got.shape == (3, rh, rw, nch) and got.dtype == refs[0].dtype
    for k in range(3):
        want = DU.box_mean_int(refs[k])
        assert (got[k] == want).all(), (k, int((got[k] != want).sum()))
    assert via_api.dtype == got.dtype and (via_api == got).all()


# ---------------------------------------------------------------- orientations
def oriented(ref, orientation):
    """EXIF orientation as displayed (test_gpu_layers.test_orientation)."""
    t = lambda x: x.transpose(1, 0, 2)
    return {1: ref, 2: ref[:, ::-1], 3: ref[::-1, ::-1], 4: ref[::-1], 5: t(ref), 6: t(ref[::-1]), 7: t(ref[::-1, ::-1]), 8: t(ref[:, ::-1])}[orientation]


@pytest.mark.parametrize("orientation", [1, 2, 3, 4, 5, 6, 7, 8])
def test_orientations(oracle, orientation):
    """21 x 10: partial cells in both directions, which lie at the far canvas edge for the flipped and transposed orientations."""
    w, h = 21, 10
    rng = np.random.default_rng(50 + orientation)
    frames = replace_frames(rng, w, h, 4, 8)
    kw = dict(lossless=True, container=False)
    canvas = oracle.encode(np.zeros((h, w, 4), np.uint8), orientation=orientation, animation_frames=2, **kw)
    layers = [LU.Layer(oracle.encode(fr.px, **kw), x0=fr.x0, y0=fr.y0, crop=fr.crop, duration=fr.duration, save_ref=fr.save,
                       blending=[LU.Blending(0, 0, False, fr.source), LU.Blending(0, 0, False, fr.source)]) for fr in frames]
    with api.Animation(LU.layered(canvas, layers)) as a:
        assert (a.info.width, a.info.height) == ((h, w) if orientation >= 5 else (w, h))
        got = thumbs(a)
        a.rewind()
        full = a.next(1).cpu().numpy()[0]
    refs = refs_of(w, h, frames, 8, True)
    assert (full == oriented(refs[0], orientation)).all()       # (the helper's orientation is the decoder's)
    for k in range(3):
        want = DU.box_mean_int(np.ascontiguousarray(oriented(refs[k], orientation)))
        assert got[k].shape == want.shape and (got[k] == want).all(), (k, int((got[k] != want).sum()))


# ---------------------------------------------------------------- blend files
@pytest.mark.parametrize("bits,premul", [(8, False), (8, True), (16, False), (16, True)])
def test_blend_files(oracle, bits, premul):
    """The full-size rule allows 1 LSB on 0.1 % of the samples against the composite; a cell holds 64 samples, so a thumbnail sample
    may differ by 1 LSB and at most 6.4 % of them do.  (The exact cases above carry the precision.)"""
    frames = mixed_frames(bits)
    with api.Animation(build(oracle, W, H, frames, bits=bits, premul=premul, animation=True)) as a:
        got = thumbs(a)
    refs = displayed = refs_of(W, H, frames, bits, True, premul)
    assert got.shape[0] == len(displayed) == 3
    for k in range(3):
        d = np.abs(got[k].astype(np.int64) - DU.box_mean_int(refs[k]).astype(np.int64))
        print("image %d: max %d LSB, %.4f of the samples differ" % (k, d.max(), (d > 0).mean()))
        assert d.max() <= 1 and (d > 0).mean() <= 0.064, (k, int(d.max()), float((d > 0).mean()))
    assert (got[0] != got[1]).any() and (got[1] != got[2]).any()


# ---------------------------------------------------------------- float files
@pytest.mark.parametrize("float_bits", [16, 32])
def test_float_files(oracle, float_bits):
    """binary16 / binary32, all-replace: against the float64 mean.  Tolerance: 2^-18 of the cell's mean |v| (a float32 sum of up to 63
    additions, each within 2^-24 of its partial sum, and the division) plus half an ulp of the output type at the result (the output
    rounding)."""
    dt = np.float16 if float_bits == 16 else np.float32
    w, h = 41, 33
    rng = np.random.default_rng(float_bits)
    px = lambda ww, hh: rng.uniform(0.0, 1.5, (hh, ww, 4)).astype(dt)
    frames = [F(px(w, h), crop=False, duration=1, save=1), F(px(25, 20), x0=20, y0=-4, duration=1, source=1, save=1),
              F(px(9, 30), x0=-3, y0=5, duration=1, source=1)]
    kw = dict(lossless=True, container=False, float_samples=float_bits, lossless_predictor=5, lossless_tree=1)
    canvas = oracle.encode(np.zeros((h, w, 4), dt), animation_frames=2, **kw)
    layers = [LU.Layer(oracle.encode(fr.px, **kw), x0=fr.x0, y0=fr.y0, crop=fr.crop, duration=fr.duration, save_ref=fr.save,
                       blending=[LU.Blending(0, 0, False, fr.source), LU.Blending(0, 0, False, fr.source)]) for fr in frames]
    with api.Animation(LU.layered(canvas, layers)) as a:
        assert a.dtype == dt
        got = thumbs(a)
    for k in range(3):
        ref = composite(w, h, frames, 0, True, False, displayed=k, float_out=dt)
        want = DU.box_mean_float(ref)
        tol = 2.0 ** -18 * DU.box_mean_float(np.abs(ref)) + np.spacing(np.abs(want).astype(dt)).astype(np.float64) / 2
        d = np.abs(got[k].astype(np.float64) - want)
        print("image %d: max error / tolerance %.3f" % (k, float((d / tol).max())))
        assert got[k].shape == want.shape and (d <= tol).all(), (k, float((d / tol).max()))


# ---------------------------------------------------------------- steps and combinations
@pytest.fixture(scope="module")
def long_file(oracle):
    frames = long_frames()
    refs = [DU.box_mean_int(r) for r in refs_of(9, 7, frames, 8, True)]
    return build(oracle, 9, 7, frames, animation=True), refs


def _check_long(got, refs, which):
    assert got.shape[0] == len(which)
    for g, j in zip(got, which):
        d = np.abs(g.astype(int) - refs[j].astype(int))
        assert d.max() <= (1 if j == 68 else 0), (j, int(d.max()))      # (image 68 is the one that blends)


@pytest.mark.parametrize("step", [1, 2, 5])
def test_steps(long_file, step):
    data, refs = long_file
    with api.Animation(data) as a:
        got = thumbs(a, 0, step)
        assert a.position == (70 - (69 % step), 70) and thumbs(a, 3, step).shape[0] == 0
        _check_long(got, refs, list(range(0, 70, step)))
        a.rewind()
        assert a.set_option("chunk_frames", 1) == 1
        assert (thumbs(a, 0, step) == got).all()                       # a cut behind every frame: the same bytes
        a.rewind()
        first = thumbs(a, 4, step)                                      # in two calls
        assert a.position[1] == 4 * step
        rest = thumbs(a, 0, step)
        assert (np.concatenate([first, rest]) == got).all()


def test_thumbnails_combine_with_seek_and_next(long_file):
    data, refs = long_file
    full = refs_of(9, 7, long_frames(), 8, True)
    with api.Animation(data) as a:
        a.seek(40)
        t = a.thumbnails(2, step=3)
        assert tuple(t.shape) == (2, 1, 2, 4) and a.position == (44, 46) and a._pos == 46
        _check_long(t.cpu().numpy(), refs, [40, 43])
        one = a.next(1).cpu().numpy()                                   # the full-size image at the stated position
        assert a.position == (47, 47)
        AU.check_images(one[0], full[46], exact=True)
        a.seek(67)
        _check_long(a.thumbnails(None, step=1).cpu().numpy(), refs, [67, 68, 69])   # image 68 reads slot 3 from frame 2
        assert a.thumbnails().shape[0] == 0
        with pytest.raises(ValueError):
            a.thumbnails(1, step=0)
        import torch
        buf = torch.zeros(2 * 8 - 1, dtype=torch.uint8, device="cuda")   # two thumbnails of 2 x 1 x 4 bytes do not fit
        n, err = C.c_int32(-1), api.ErrorInfo()
        a.seek(3)
        st = a._L.jxlhip_animation_next_reduced(a._h, 1, 0, buf.data_ptr(), buf.numel(), C.byref(n), C.byref(err))
        assert api.DECODER_STATUS[st] == "InvalidParameter" and b"step" in err.errorMessage and a.position[1] == 3
        a.rewind()
        st = a._L.jxlhip_animation_next_reduced(a._h, 2, 1, buf.data_ptr(), buf.numel(), C.byref(n), C.byref(err))
        assert api.DECODER_STATUS[st] == "InvalidParameter" and n.value == 0 and b"15 bytes, 2 displayed images at 1:8 need 16" in err.errorMessage
        assert a.position == (0, 0)


def test_thumbnails_of_the_keyed_file(oracle):
    """Entry points in the middle, zero-duration layers, slots 1 and 2: seek, then every second image."""
    frames = SU.keyed_frames()
    refs = [DU.box_mean_int(r) for r in refs_of(SU.KW, SU.KH, frames, 8, True)]
    with api.Animation(build(oracle, SU.KW, SU.KH, frames, animation=True)) as a:
        a.seek(5)
        got = thumbs(a, 0, 2)
        assert got.shape[0] == 4 and a.position[1] == 12
        for g, j in zip(got, (5, 7, 9, 11)):
            d = np.abs(g.astype(int) - refs[j].astype(int))
            assert d.max() <= 1 and (d > 0).mean() <= 0.064, (j, int(d.max()))


# ---------------------------------------------------------------- single-frame files
def test_single_frame_files(oracle):
    rng = np.random.default_rng(12)
    img = _px(rng, 50, 33)
    lossless = oracle.encode(img, lossless=True)
    lossy = oracle.encode(synth(70, 50, 3), distance=1.0)
    rotated = oracle.encode(img, lossless=True, orientation=6)
    import icc_util
    five = _px(rng, 20, 10, 5)                                    # CMYK and alpha: five samples per pixel
    cmyk = oracle.encode(five, lossless=True, icc=icc_util.cmyk_profile(), cmyk=True)
    inks = five.copy()
    inks[..., :4] = 255 - inks[..., :4]                           # CMYK inks leave inverted (0 = no ink), as test_gpu_icc states
    for data, full in ((lossless, img), (lossy, api.load_image(lossy).pixels), (rotated, oriented(img, 6)), (cmyk, inks)):
        with api.Animation(data) as a:
            assert a.info.num_displayed == 1 and a.entry_points == [0]
            got = thumbs(a)
            assert a.position[1] == 1 and thumbs(a).shape[0] == 0
            again = a.read_thumbnails()
        want = DU.box_mean_int(np.ascontiguousarray(full))
        assert got.shape == (1,) + want.shape and (got[0] == want).all() and (again == got).all()
