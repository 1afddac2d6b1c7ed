"""Layered stills on the GPU: frames blended onto the canvas (compose_kernel), checked against a numpy f32 composite of the SOURCE
layers under the rules of DESIGN.md §2 (no oracle: it cannot read layered files)."""
import numpy as np
import pytest

import layer_util as LU
from pdn_jpegxl_amd import api

pytestmark = pytest.mark.gpu


class F:
    """One frame as the reference composite sees it: source pixels, placement, blending, save slot."""

    def __init__(self, px, x0=0, y0=0, crop=True, mode=0, clamp=False, source=0, amode=None, asource=None, save=0, duration=0, name=b""):
        self.px, self.x0, self.y0, self.crop = px, x0, y0, crop
        self.mode, self.clamp, self.source = mode, clamp, source
        self.amode = mode if amode is None else amode
        self.asource = source if asource is None else asource
        self.save, self.duration, self.name = save, duration, name


def composite(w, h, frames, bits, has_alpha, premul, displayed=None, float_out=None):
    """numpy f32 composite; frames saved per the rule of the header (not is_last, and duration 0 or a save slot).  float_out: the
    frames are float samples and the result leaves as that dtype (float16 / float32)."""
    nch = frames[0].px.shape[2]
    ai = nch - 1 if has_alpha else -1
    unit = np.float32(1) if float_out else np.float32(1.0 / ((1 << bits) - 1))
    slots = [np.zeros((h, w, nch), np.float32) for _ in range(4)]
    displayed = len(frames) - 1 if displayed is None else displayed
    res = None
    for k, fr in enumerate(frames[:displayed + 1]):
        oc, oa = slots[fr.source], slots[fr.asource]
        res = oc.copy()
        if ai >= 0:
            res[..., ai] = oa[..., ai]
        new = fr.px.astype(np.float32) * unit
        fh, fw = new.shape[:2]
        x0, y0 = (fr.x0, fr.y0) if fr.crop else (0, 0)
        cx0, cy0, cx1, cy1 = max(0, x0), max(0, y0), min(w, x0 + fw), min(h, y0 + fh)
        if cx0 < cx1 and cy0 < cy1:
            nw = new[cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0]
            r = res[cy0:cy1, cx0:cx1]
            ocr, oar = oc[cy0:cy1, cx0:cx1], oa[cy0:cy1, cx0:cx1]
            for c in range(nch):
                is_a = c == ai
                mode, clamp = (fr.amode, fr.clamp) if is_a else (fr.mode, fr.clamp)
                a = nw[..., ai] if ai >= 0 else np.ones(nw.shape[:2], np.float32)
                if clamp:
                    a = np.clip(a, 0, 1)
                old = oar[..., c] if is_a else ocr[..., c]
                ob = (oar if is_a else ocr)[..., ai] if ai >= 0 else 0
                n = nw[..., c]
                one = np.float32(1)
                if mode == 0:
                    v = n
                elif mode == 1:
                    v = old + n
                elif mode == 2:
                    if is_a:
                        v = a + ob * (one - a)
                    elif premul:
                        v = n + old * (one - a)
                    else:
                        A = a + ob * (one - a)
                        with np.errstate(divide="ignore", invalid="ignore"):
                            v = np.where(A == 0, np.float32(0), (n * a + old * ob * (one - a)) / A)
                elif mode == 3:
                    v = old if is_a else old + n * a
                else:
                    v = old * (np.clip(n, 0, 1) if clamp else n)
                r[..., c] = v
        is_last = k == len(frames) - 1
        if not is_last and (fr.duration == 0 or fr.save != 0):
            slots[fr.save] = res.copy()
    if premul and ai >= 0:
        res[..., :ai] *= np.float32(1) / np.maximum(np.float32(2.0 ** -26), res[..., ai:ai + 1])
    if float_out:
        return res.astype(float_out)
    top = np.float32((1 << (16 if bits > 8 else 8)) - 1)
    f = res * top
    out = np.where(~(f > 0), 0, np.where(f >= top, top, np.floor(f + np.float32(0.5))))
    return out.astype(np.uint16 if bits > 8 else np.uint8)


def build(oracle, w, h, frames, bits=8, premul=False, animation=False, extra_after=None):
    """A layered file of the frames (each encoded losslessly on its own) on a w x h canvas."""
    kw = dict(lossless=True, container=False, bits=bits, premultiplied_alpha=premul)
    nch = frames[0].px.shape[2]
    canvas = oracle.encode(np.zeros((h, w, nch), frames[0].px.dtype), animation_frames=2 if animation else 1, **kw)
    nec = 1 if nch in (2, 4) else 0
    layers = []
    for fr in frames + ([extra_after] if extra_after else []):
        bl = [LU.Blending(fr.mode, 0, fr.clamp, fr.source)] + [LU.Blending(fr.amode, 0, fr.clamp, fr.asource) for _ in range(nec)]
        layers.append(LU.Layer(oracle.encode(fr.px, **kw), x0=fr.x0, y0=fr.y0, crop=fr.crop, blending=bl, duration=fr.duration,
                               save_ref=fr.save, name=fr.name))
    return LU.layered(canvas, layers)


def _px(rng, w, h, nch, bits):
    return rng.integers(0, 1 << bits, (h, w, nch), dtype=np.uint8 if bits <= 8 else np.uint16)


def _check(got, ref, exact):
    d = np.abs(got.astype(np.int64) - ref.astype(np.int64))
    if exact:
        assert d.max() == 0, (int(d.max()), int((d > 0).sum()))
    else:
        assert d.max() <= 1 and (d > 0).mean() <= 0.001, (int(d.max()), float((d > 0).mean()))


@pytest.mark.parametrize("nch", [2, 4])
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("premul", [False, True])
@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_lossless_every_blend_mode(oracle, mode, clamp, premul, bits, nch):
    rng = np.random.default_rng(100 * mode + 10 * bits + nch + 2 * clamp + premul)
    W, H = 67, 45
    frames = [F(_px(rng, W, H, nch, bits), crop=False), F(_px(rng, 40, 30, nch, bits), x0=-7, y0=20, mode=mode, clamp=clamp)]
    f = build(oracle, W, H, frames, bits=bits, premul=premul)
    got = api.load_image(f)
    assert got.trace.count("setLayerData") == 1 and got.pixels.shape == (H, W, nch)
    _check(got.pixels, composite(W, H, frames, bits, True, premul), exact=mode in (0, 1))


@pytest.mark.parametrize("float_bits", [16, 32])
@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_float_layers_with_samples_outside_unit_range(oracle, mode, clamp, float_bits):
    """Float samples (binary16 / binary32) above 1: `clamp` changes the blending alpha (and, for kMul, the new sample)."""
    rng = np.random.default_rng(1000 + 10 * mode + clamp + float_bits)
    dt = np.float16 if float_bits == 16 else np.float32
    W, H = 41, 33
    # (above 1 only: float32 Modular streams of negative samples - bit patterns with the sign set - are not decoded on the GPU path, a
    # limit of the single-frame decode as well)
    px = lambda w, h: rng.uniform(0.0, 1.5, (h, w, 4)).astype(dt)
    frames = [F(px(W, H), crop=False), F(px(25, 20), x0=20, y0=-4, mode=mode, clamp=clamp)]
    kw = dict(lossless=True, container=False, float_samples=float_bits, lossless_predictor=5, lossless_tree=1)
    canvas = oracle.encode(np.zeros((H, W, 4), dt), **kw)
    layers = [LU.Layer(oracle.encode(fr.px, **kw), x0=fr.x0, y0=fr.y0, crop=fr.crop,
                       blending=[LU.Blending(fr.mode, 0, fr.clamp, 0), LU.Blending(fr.mode, 0, fr.clamp, 0)]) for fr in frames]
    got = api.load_image(LU.layered(canvas, layers)).pixels
    ref = composite(W, H, frames, 0, True, False, float_out=dt)
    assert got.dtype == dt and got.shape == ref.shape
    g, r = got.astype(np.float64), ref.astype(np.float64)
    # (the kernel may contract multiply-adds: kBlend divides by A = a + ob * (1 - a), which unclamped alphas can bring near 0, so a few
    # samples may differ by more than rounding; ignoring `clamp` would move about half of the crop's samples)
    tol = np.abs(r) * (2.0 ** -9 if float_bits == 16 else 2.0 ** -20) + 1e-6
    assert (np.abs(g - r) > tol).mean() <= 0.002, float((np.abs(g - r) > tol).mean())
    if mode == 0 or mode == 1:
        assert (got.view(np.uint16 if float_bits == 16 else np.uint32) == ref.view(np.uint16 if float_bits == 16 else np.uint32)).all()


def test_lossy_replace_layers_equal_their_standalone_decodes(oracle):
    """Lossy (XYB) kReplace layers with crops: byte-identical to a numpy composite of LoadImage of each layer file on its own (every
    frame decodes and filters on its own, so there is no tolerance)."""
    from pdn_jpegxl_amd.synth import synth
    W, H = 333, 257
    parts = [(synth(W, H, 21), None), (synth(150, 120, 22), (-30, 40)), (synth(90, 200, 23), (280, 100)), (synth(64, 64, 24), (100, -10))]
    files = [oracle.encode(img, distance=1.0, container=False) for img, _ in parts]
    layers = [LU.Layer(cs, crop=pos is not None, x0=pos[0] if pos else 0, y0=pos[1] if pos else 0) for cs, (_, pos) in zip(files, parts)]
    got = api.load_image(LU.layered(files[0], layers)).pixels
    ref = np.zeros((H, W, 4), np.uint8)
    for cs, (_, pos) in zip(files, parts):
        alone = api.load_image(cs).pixels
        x0, y0 = pos if pos else (0, 0)
        h, w = alone.shape[:2]
        cx0, cy0, cx1, cy1 = max(0, x0), max(0, y0), min(W, x0 + w), min(H, y0 + h)
        ref[cy0:cy1, cx0:cx1] = alone[cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0]
    assert got.shape == ref.shape and (got == ref).all(), int((got != ref).sum())


@pytest.mark.parametrize("nch", [1, 3])
def test_lossless_layers_without_alpha(oracle, nch):
    rng = np.random.default_rng(nch)
    frames = [F(_px(rng, 50, 40, nch, 8), crop=False), F(_px(rng, 20, 10, nch, 8), x0=30, y0=35, mode=1), F(_px(rng, 9, 9, nch, 8), x0=-3, y0=-4, mode=4)]
    got = api.load_image(build(oracle, 50, 40, frames))
    _check(got.pixels.reshape(40, 50, nch), composite(50, 40, frames, 8, False, False), exact=False)


def test_lossless_geometry(oracle):
    """Crops off every edge, negative offsets, 1-pixel-wide crops, a frame larger than the canvas, a canvas that is a multiple of
    neither 8 nor the group size (and spans several groups)."""
    rng = np.random.default_rng(7)
    W, H = 301, 267
    frames = [F(_px(rng, W, H, 4, 8), crop=False)]
    for (x0, y0, w, h) in [(-10, 50, 30, 40), (290, 100, 40, 20), (100, -5, 20, 15), (120, 260, 10, 30), (-3, -3, 1, 300),
                           (200, 7, 1, 1), (-20, -20, 340, 310), (33, 44, 257, 1)]:
        frames.append(F(_px(rng, w, h, 4, 8), x0=x0, y0=y0, mode=2))
    f = build(oracle, W, H, frames)
    _check(api.load_image(f).pixels, composite(W, H, frames, 8, True, False), exact=False)


def test_slots(oracle):
    """A layer blends onto slot 1 while slot 0 holds something else; a saved-then-overwritten slot."""
    rng = np.random.default_rng(9)
    W, H = 64, 50
    A, B_ = _px(rng, W, H, 4, 8), _px(rng, W, H, 4, 8)
    frames = [F(A, crop=False, save=1), F(B_, crop=False, save=0), F(_px(rng, 30, 20, 4, 8), x0=10, y0=5, mode=2, source=1)]
    got = api.load_image(build(oracle, W, H, frames)).pixels
    ref = composite(W, H, frames, 8, True, False)
    _check(got, ref, exact=False)
    assert (got[30:, :] == A[30:, :]).all()   # outside the crop: slot 1 (A), not the last saved frame (B)
    frames = [F(A, crop=False), F(B_, crop=False), F(_px(rng, 30, 20, 4, 8), x0=10, y0=5, mode=1)]
    got = api.load_image(build(oracle, W, H, frames)).pixels
    _check(got, composite(W, H, frames, 8, True, False), exact=True)
    assert (got[30:, :] == B_[30:, :]).all()


def test_animation_first_displayed_image(oracle):
    """Two zero-duration layers and a frame with a duration make the first displayed image; the next displayed image is ignored, and
    setLayerData is called once, with the displayed frame's name."""
    rng = np.random.default_rng(11)
    W, H = 48, 40
    frames = [F(_px(rng, W, H, 4, 8), crop=False), F(_px(rng, 20, 20, 4, 8), x0=5, y0=5, mode=2),
              F(_px(rng, 10, 30, 4, 8), x0=30, y0=3, mode=1, duration=7, name=b"shown")]
    later = F(_px(rng, W, H, 4, 8), crop=False, name=b"later")
    got = api.load_image(build(oracle, W, H, frames, animation=True, extra_after=later))
    assert got.trace.count("setLayerData") == 1 and got.layer_name == "shown"
    # the displayed frame is not is_last here: nothing is saved after it, so the reference composite is the same
    _check(got.pixels, composite(W, H, frames, 8, True, False), exact=False)


@pytest.mark.parametrize("orientation", range(1, 9))
def test_orientation(oracle, orientation):
    rng = np.random.default_rng(orientation)
    W, H = 37, 23
    frames = [F(_px(rng, W, H, 4, 8), crop=False), F(_px(rng, 15, 9, 4, 8), x0=20, y0=-2, mode=2)]
    kw = dict(lossless=True, container=False)
    canvas = oracle.encode(np.zeros((H, W, 4), np.uint8), orientation=orientation, **kw)
    layers = [LU.Layer(oracle.encode(fr.px, **kw), x0=fr.x0, y0=fr.y0, crop=fr.crop,
                       blending=[LU.Blending(fr.mode, 0, False, 0), LU.Blending(fr.mode, 0, False, 0)]) for fr in frames]
    got = api.load_image(LU.layered(canvas, layers)).pixels
    ref = composite(W, H, frames, 8, True, False)
    # EXIF orientation as displayed: 2 mirror, 3 rotate 180, 4 flip, 5 transpose, 6 rotate 90 cw, 7 transverse, 8 rotate 90 ccw
    o = {1: ref, 2: ref[:, ::-1], 3: ref[::-1, ::-1], 4: ref[::-1], 5: ref.transpose(1, 0, 2), 6: ref[::-1].transpose(1, 0, 2),
         7: ref[::-1, ::-1].transpose(1, 0, 2), 8: ref[:, ::-1].transpose(1, 0, 2)}[orientation]
    _check(got, o, exact=False)


def test_batch_mixes_layered_and_single_frame_files(oracle, gpu_decoder):
    import torch
    rng = np.random.default_rng(13)
    singles = [oracle.encode(_px(rng, 70, 50, 4, 8), lossless=True), oracle.encode(_px(rng, 120, 90, 4, 8), distance=1.0)]
    frames = [F(_px(rng, 60, 40, 4, 8), crop=False), F(_px(rng, 20, 20, 4, 8), x0=50, y0=30, mode=2)]
    lay = build(oracle, 60, 40, frames)
    # a layer whose section bytes are damaged: the host parse passes, the GPU flags that frame, and only its file fails
    from pdn_jpegxl_amd.synth import synth
    kw = dict(lossless=True, container=False, lossless_tree=1, lossless_predictor=5)
    bad_layer = oracle.encode(synth(300, 280, 7), **kw)
    corrupt = bytearray(LU.layered(oracle.encode(np.zeros((300, 320, 4), np.uint8), **kw),
                                   [LU.Layer(oracle.encode(synth(320, 300, 3), **kw), crop=False), LU.Layer(bad_layer, x0=10, y0=10)]))
    mid = len(corrupt) - (len(bad_layer) - LU.read_image_header(bad_layer).frame_start) // 2
    corrupt[mid] ^= 0x55
    corrupt[mid + 1] ^= 0xAA
    corrupt = bytes(corrupt)
    assert api.parse_check(corrupt)[0] == "Ok"
    files = [singles[0], lay, singles[1], corrupt, lay]

    def run(batch):
        shapes = [(api.peek(f).height, api.peek(f).width, api.peek(f).num_channels) for f in batch]
        outs = [torch.zeros(int(np.prod(s)), dtype=torch.uint8, device="cuda") for s in shapes]
        torch.cuda.synchronize()
        st = gpu_decoder.decode_batch(batch, [o.data_ptr() for o in outs], raise_on_error=False)
        return st, [o.cpu().numpy().reshape(s) for o, s in zip(outs, shapes)]

    st, got = run(files)
    assert st[0] == 0 and st[1] == 0 and st[2] == 0 and st[4] == 0 and st[3] != 0, st
    assert "GPU decode failed" in gpu_decoder.last_error and "image 3," in gpu_decoder.last_error, gpu_decoder.last_error
    one = api.load_image(lay).pixels
    assert (got[1] == one).all() and (got[4] == one).all()
    st2, alone = run(singles)
    assert st2 == [0, 0]
    assert (alone[0] == got[0]).all() and (alone[1] == got[2]).all()


@pytest.mark.parametrize("case,needle", [
    ("lossy_blend", "blend modes other than replace on lossy (XYB) frames"),
    ("reference_only", "reference-only frames are not supported yet (layered image, frame 0)"),
    ("upsampled", "upsampled frames are not supported yet (layered image, frame 0)"),
])
def test_refusals_through_the_abi(oracle, case, needle):
    rng = np.random.default_rng(17)
    kw = dict(lossless=True, container=False)
    canvas = oracle.encode(_px(rng, 40, 30, 4, 8), **kw)
    small = oracle.encode(_px(rng, 10, 10, 4, 8), **kw)
    if case == "lossy_blend":
        lc = oracle.encode(_px(rng, 40, 30, 4, 8), distance=1.0, container=False)
        f = LU.layered(lc, [LU.Layer(oracle.encode(_px(rng, 10, 10, 4, 8), distance=1.0, container=False), x0=2, y0=2,
                                     blending=[LU.Blending(2, 0, False, 0), LU.Blending(2, 0, False, 0)])])
    elif case == "reference_only":
        f = LU.layered(canvas, [LU.Layer(canvas, crop=False, frame_type=2), LU.Layer(small, x0=1, y0=1)])
    else:
        f = LU.layered(canvas, [LU.Layer(canvas, crop=False, upsampling2=True), LU.Layer(small, x0=1, y0=1)])
    with pytest.raises(api.FormatError) as e:
        api.load_image(f)
    assert needle in str(e.value)


def test_band_decode_of_a_layered_file_is_refused(oracle, gpu_decoder):
    import torch
    rng = np.random.default_rng(19)
    frames = [F(_px(rng, 60, 40, 4, 8), crop=False), F(_px(rng, 20, 20, 4, 8), x0=5, y0=5, mode=2)]
    f = build(oracle, 60, 40, frames)
    out = torch.zeros(60 * 40 * 4, dtype=torch.uint8, device="cuda")
    gpu_decoder.set_option("band_first_row", 0)
    gpu_decoder.set_option("band_rows", 1)
    try:
        st = gpu_decoder.decode_batch([f], [out.data_ptr()], raise_on_error=False)
        assert st[0] != 0 and "band decode of a layered image" in gpu_decoder.last_error
    finally:
        gpu_decoder.set_option("band_rows", 0)
