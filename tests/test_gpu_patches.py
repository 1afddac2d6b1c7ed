"""Patches on the GPU (patch_kernel): reference-only atlas frames and patch dictionaries.

Ground truth first: an image T whose glyphs are zeroed in the coded frame and restored by Replace patches, or kept as a background B
with Add patches of P where T = B + P; the decode must equal T byte for byte whatever the blend formulas are.  The other modes are
checked against a numpy f32 restatement of DESIGN.md §2 (tolerances as tests/test_gpu_layers.py)."""
import numpy as np
import pytest

import layer_util as LU
import patch_util as PU
from pdn_jpegxl_amd import api

pytestmark = pytest.mark.gpu

KW = dict(lossless=True, container=False)


def _rec(mode, clamp=False):
    return (mode, 0, clamp)


def glyph_scene(rng, W, H, nch, dtype, top, gw=7, gh=9, nglyph=5, step=(11, 13), margin=1):
    """A screen-content image: flat background, glyphs of `nglyph` kinds on a grid (each kind used several times), the atlas that holds
    one of each kind side by side, and the dictionary placing them (one reference patch per kind)."""
    bg = np.zeros((H, W, nch), dtype)
    bg[...] = rng.integers(0, top // 2 + 1, nch).astype(dtype)
    glyphs = [rng.integers(0, top // 2 + 1, (gh, gw, nch)).astype(dtype) for _ in range(nglyph)]
    atlas = np.zeros((gh + 2, nglyph * (gw + 1) + 1, nch), dtype)
    for g in range(nglyph):
        atlas[1:1 + gh, 1 + g * (gw + 1):1 + g * (gw + 1) + gw] = glyphs[g]
    places = [[] for _ in range(nglyph)]
    k = 0
    for y in range(margin, H - gh + 1, step[1]):
        for x in range(margin, W - gw + 1, step[0]):
            places[k % nglyph].append((x, y))
            k += 1
    return bg, glyphs, atlas, places


def replace_case(rng, W, H, nch, dtype, top):
    """(T, the coded frame with every glyph zeroed, atlas, places, glyph size)."""
    bg, glyphs, atlas, places = glyph_scene(rng, W, H, nch, dtype, top)
    T, coded = bg.copy(), bg.copy()
    gh, gw = glyphs[0].shape[:2]
    for g, pl in enumerate(places):
        for x, y in pl:
            T[y:y + gh, x:x + gw] = glyphs[g]
            coded[y:y + gh, x:x + gw] = 0
    return T, coded, atlas, places, (gw, gh)


def refs_for(places, size, nec, mode, slot=0):
    gw, gh = size
    return [PU.Ref(slot, 1 + g * (gw + 1), 1, gw, gh, [PU.Place(x, y, [_rec(mode)] * (1 + nec)) for x, y in pl])
            for g, pl in enumerate(places) if pl]


def build_patched(oracle, canvas_px, coded, atlas, refs, nec, enc_kw, orientation=1):
    canvas = oracle.encode(np.zeros_like(canvas_px), orientation=orientation, **enc_kw)
    pf = PU.patched(oracle.encode(coded, **enc_kw), refs, nec)
    return LU.layered(canvas, [LU.Layer(oracle.encode(atlas, **enc_kw), frame_type=2, save_before_ct=True), LU.Layer(pf, crop=False, flags=2)])


@pytest.mark.parametrize("kind", ["u8", "u16", "f16", "f32"])
@pytest.mark.parametrize("nch", [3, 4])
def test_replace_patches_restore_the_image(oracle, kind, nch):
    rng = np.random.default_rng(10 * nch + len(kind))
    W, H = 173, 91
    dtype, top, enc = {"u8": (np.uint8, 255, dict(KW)), "u16": (np.uint16, 65535, dict(KW, bits=16)),
                       "f16": (np.float16, 1, dict(KW, float_samples=16, lossless_predictor=5, lossless_tree=1)),
                       "f32": (np.float32, 1, dict(KW, float_samples=32, lossless_predictor=5, lossless_tree=1))}[kind]
    if kind in ("f16", "f32"):
        bg, glyphs, atlas, places = glyph_scene(rng, W, H, nch, np.uint8, 255)
        to_f = lambda a: (a.astype(np.float32) / 255).astype(dtype)
        T, coded = to_f(bg), to_f(bg)
        gh, gw = glyphs[0].shape[:2]
        for g, pl in enumerate(places):
            for x, y in pl:
                T[y:y + gh, x:x + gw] = to_f(glyphs[g])
                coded[y:y + gh, x:x + gw] = 0
        atlas, size = to_f(atlas), (gw, gh)
    else:
        T, coded, atlas, places, size = replace_case(rng, W, H, nch, dtype, top)
    nec = 1 if nch == 4 else 0
    f = build_patched(oracle, T, coded, atlas, refs_for(places, size, nec, PU.REPLACE), nec, enc)
    got = api.load_image(f).pixels.reshape(H, W, nch)
    assert got.dtype == T.dtype and (got == T).all(), int((got != T).sum())


@pytest.mark.parametrize("bits", [8, 16])
def test_add_patches_reach_the_image(oracle, bits):
    """T = B + P: the coded frame keeps the background B under every glyph, the atlas holds P."""
    rng = np.random.default_rng(50 + bits)
    W, H = 130, 77
    dtype, top = (np.uint8, 255) if bits == 8 else (np.uint16, 65535)
    bg, glyphs, atlas, places = glyph_scene(rng, W, H, 4, dtype, top)
    T = bg.copy()
    gh, gw = glyphs[0].shape[:2]
    for g, pl in enumerate(places):
        for x, y in pl:
            T[y:y + gh, x:x + gw] = bg[y:y + gh, x:x + gw] + glyphs[g]
    enc = dict(KW, bits=bits)
    f = build_patched(oracle, T, bg, atlas, refs_for(places, (gw, gh), 1, PU.ADD), 1, enc)
    got = api.load_image(f).pixels
    assert (got == T).all(), int((got != T).sum())


@pytest.mark.parametrize("orientation", range(1, 9))
def test_orientations(oracle, orientation):
    rng = np.random.default_rng(70 + orientation)
    W, H = 61, 40
    T, coded, atlas, places, size = replace_case(rng, W, H, 4, np.uint8, 255)
    f = build_patched(oracle, T, coded, atlas, refs_for(places, size, 1, PU.REPLACE), 1, KW, orientation=orientation)
    got = api.load_image(f).pixels
    o = {1: T, 2: T[:, ::-1], 3: T[::-1, ::-1], 4: T[::-1], 5: T.transpose(1, 0, 2), 6: T[::-1].transpose(1, 0, 2),
         7: T[::-1, ::-1].transpose(1, 0, 2), 8: T[:, ::-1].transpose(1, 0, 2)}[orientation]
    assert got.shape == o.shape and (got == o).all(), int((got != o).sum())


# ---------------------------------------------------------------- restated rules (numpy f32)
def patch_sample(mode, is_alpha, premul, clamp, nw, an, old, ao):
    one = np.float32(1)
    if mode == 0:
        return old
    if mode == 1:
        return nw
    if mode == 2:
        return old + nw
    if mode == 3:
        return old * (np.clip(nw, 0, 1) if clamp else nw)
    below = mode in (5, 7)
    n, o = (old, nw) if below else (nw, old)
    a, ob = (ao, an) if below else (an, ao)
    if clamp:
        a = np.clip(a, 0, 1)
    if mode in (4, 5):
        if is_alpha:
            return a + ob * (one - a)
        if premul:
            return n + o * (one - a)
        A = a + ob * (one - a)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(A == 0, np.float32(0), (n * a + o * ob * (one - a)) / A)
    return o if is_alpha else o + n * a


def apply_patches(frame, atlases, refs, has_alpha, premul):
    """frame: f32 (h, w, nch), updated in dictionary order; atlases: {slot: f32 array}."""
    nch = frame.shape[2]
    ai = nch - 1 if has_alpha else -1
    for r in refs:
        at = atlases[r.slot][r.y0:r.y0 + r.h, r.x0:r.x0 + r.w]
        for p in r.places:
            old = frame[p.y:p.y + r.h, p.x:p.x + r.w].copy()
            ao = old[..., ai] if ai >= 0 else np.float32(1)
            an = at[..., ai] if ai >= 0 else np.float32(1)
            for c in range(nch):
                g = 1 if c == ai else 0
                mode, _, clamp = p.blend[g]
                frame[p.y:p.y + r.h, p.x:p.x + r.w, c] = patch_sample(mode, c == ai, premul, clamp, at[..., c], an, old[..., c], ao)
    return frame


def to_out(res, bits, has_alpha, premul):
    res = res.copy()
    if premul and has_alpha:
        res[..., :-1] *= np.float32(1) / np.maximum(np.float32(2.0 ** -26), res[..., -1:])
    top = np.float32((1 << (16 if bits > 8 else 8)) - 1)
    f = res * top
    out = np.where(~(f > 0), 0, np.where(f >= top, top, np.floor(f + np.float32(0.5))))
    return out.astype(np.uint16 if bits > 8 else np.uint8)


def unit(px, bits):
    return px.astype(np.float32) * np.float32(1.0 / ((1 << bits) - 1))


def _check(got, ref, exact):
    d = np.abs(got.astype(np.int64) - ref.astype(np.int64))
    if exact:
        assert d.max() == 0, (int(d.max()), int((d > 0).sum()))
    else:
        assert d.max() <= 1 and (d > 0).mean() <= 0.001, (int(d.max()), float((d > 0).mean()))


def _px(rng, w, h, nch, bits):
    return rng.integers(0, 1 << bits, (h, w, nch), dtype=np.uint8 if bits <= 8 else np.uint16)


def run_rules(oracle, W, H, frame_px, atlas_pxs, refs, bits=8, premul=False):
    """Atlases in their slots (dict slot -> pixels), one full-canvas patched frame: decode and numpy reference."""
    nch = frame_px.shape[2]
    has_alpha = nch in (2, 4)
    nec = 1 if has_alpha else 0
    kw = dict(KW, bits=bits, premultiplied_alpha=premul)
    canvas = oracle.encode(np.zeros_like(frame_px), **kw)
    layers = [LU.Layer(oracle.encode(px, **kw), frame_type=2, save_ref=s) for s, px in atlas_pxs.items()]
    layers.append(LU.Layer(PU.patched(oracle.encode(frame_px, **kw), refs, nec), crop=False, flags=2))
    got = api.load_image(LU.layered(canvas, layers)).pixels.reshape(H, W, nch)
    ref = apply_patches(unit(frame_px, bits), {s: unit(px, bits) for s, px in atlas_pxs.items()}, refs, has_alpha, premul)
    return got, to_out(ref, bits, has_alpha, premul)


@pytest.mark.parametrize("premul", [False, True])
@pytest.mark.parametrize("mode,clamp", [(PU.NONE, False)] + [(m, c) for m in (PU.MUL, PU.BLEND_ABOVE, PU.BLEND_BELOW, PU.AWADD_ABOVE, PU.AWADD_BELOW)
                                                             for c in (False, True)])
def test_every_patch_mode(oracle, mode, clamp, premul):
    rng = np.random.default_rng(200 + 10 * mode + 2 * clamp + premul)
    W, H = 70, 52
    frame, atlas = _px(rng, W, H, 4, 8), _px(rng, 40, 30, 4, 8)
    # colour and alpha records differ; the positions overlap (order matters), touch the right and bottom edges, and include 1 x 1
    other = PU.REPLACE if mode != PU.REPLACE else PU.ADD
    refs = [PU.Ref(0, 3, 2, 20, 15, [PU.Place(5, 5, [_rec(mode, clamp), _rec(other)]), PU.Place(12, 9, [_rec(mode, clamp), _rec(mode, clamp)]),
                                     PU.Place(W - 20, H - 15, [_rec(mode, clamp), _rec(PU.NONE)])]),
            PU.Ref(0, 39, 29, 1, 1, [PU.Place(W - 1, 0, [_rec(mode, clamp)] * 2), PU.Place(0, H - 1, [_rec(mode, clamp)] * 2)])]
    got, ref = run_rules(oracle, W, H, frame, {0: atlas}, refs, premul=premul)
    _check(got, ref, exact=mode == PU.NONE)


def test_overlap_order_several_atlases_u16(oracle):
    """Four atlases in slots 0-3, positions that overlap (the later one is blended onto the earlier result), u16 samples, and a frame
    whose patched rows cross 64x64 tile edges."""
    rng = np.random.default_rng(300)
    W, H = 150, 140
    frame = _px(rng, W, H, 4, 16)
    atlases = {s: _px(rng, 30 + 10 * s, 20 + 5 * s, 4, 16) for s in range(4)}
    refs = [PU.Ref(s, s, s, 25, 18, [PU.Place(50 + 3 * s, 55 + 2 * s, [_rec(m)] * 2) for m in (PU.REPLACE, PU.ADD)]) for s in range(4)]
    refs.append(PU.Ref(2, 0, 0, 50, 30, [PU.Place(60, 60, [_rec(PU.BLEND_ABOVE), _rec(PU.BLEND_ABOVE)]), PU.Place(100, 110, [_rec(PU.MUL, True)] * 2)]))
    got, ref = run_rules(oracle, W, H, frame, atlases, refs, bits=16)
    _check(got, ref, exact=False)


@pytest.mark.parametrize("nch", [1, 2, 3])
def test_other_channel_counts(oracle, nch):
    rng = np.random.default_rng(400 + nch)
    W, H = 66, 70
    frame, atlas = _px(rng, W, H, nch, 8), _px(rng, 20, 20, nch, 8)
    nec = 1 if nch == 2 else 0
    mode = PU.BLEND_ABOVE if nec else PU.ADD
    refs = [PU.Ref(1, 2, 2, 10, 12, [PU.Place(55 - 5 * k, 3 + 6 * k, [_rec(PU.REPLACE if k % 2 else mode)] * (1 + nec)) for k in range(10)])]
    got, ref = run_rules(oracle, W, H, frame, {1: atlas}, refs)
    _check(got, ref, exact=nec == 0)


def test_cropped_atlas_and_cropped_patched_layer(oracle):
    """The atlas is a cropped reference-only frame (its own size); the patched frame is a cropped layer that blends (kBlend) onto the
    canvas saved in slot 1, while the atlas sits in slot 0."""
    rng = np.random.default_rng(500)
    W, H = 90, 70
    base, layer, atlas = _px(rng, W, H, 4, 8), _px(rng, 40, 30, 4, 8), _px(rng, 25, 16, 4, 8)
    refs = [PU.Ref(0, 5, 3, 20, 13, [PU.Place(0, 0, [_rec(PU.REPLACE)] * 2), PU.Place(20, 17, [_rec(PU.ADD)] * 2)])]
    canvas = oracle.encode(np.zeros_like(base), **KW)
    blend = [LU.Blending(2, 0, False, 1), LU.Blending(2, 0, False, 1)]
    f = LU.layered(canvas, [LU.Layer(oracle.encode(atlas, **KW), frame_type=2, x0=0, y0=0), LU.Layer(oracle.encode(base, **KW), crop=False, save_ref=1),
                            LU.Layer(PU.patched(oracle.encode(layer, **KW), refs, 1), x0=60, y0=-10, flags=2, blending=blend)])
    got = api.load_image(f).pixels
    lay = apply_patches(unit(layer, 8), {0: unit(atlas, 8)}, refs, True, False)
    res = unit(base, 8)
    x0, y0 = 60, -10
    cx0, cy0, cx1, cy1 = max(0, x0), max(0, y0), min(W, x0 + 40), min(H, y0 + 30)
    nw, old = lay[cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0], res[cy0:cy1, cx0:cx1].copy()
    a, ob, one = nw[..., 3], old[..., 3], np.float32(1)
    A = a + ob * (one - a)
    for c in range(3):
        with np.errstate(divide="ignore", invalid="ignore"):
            res[cy0:cy1, cx0:cx1, c] = np.where(A == 0, np.float32(0), (nw[..., c] * a + old[..., c] * ob * (one - a)) / A)
    res[cy0:cy1, cx0:cx1, 3] = A
    _check(got, to_out(res, 8, True, False), exact=False)


def test_mixed_batch_and_band_refusal(oracle, gpu_decoder):
    """About ten files in one batch through the batch API: patched files next to plain and layered ones; the plain files' outputs equal
    their lone decodes, the patched ones their ground truth.  Band decode of a patched file is refused with its own message."""
    import torch
    rng = np.random.default_rng(600)
    files, truth = [], []
    for k in range(4):
        W, H = 90 + 13 * k, 60 + 7 * k
        T, coded, atlas, places, size = replace_case(rng, W, H, 4, np.uint8, 255)
        files.append(build_patched(oracle, T, coded, atlas, refs_for(places, size, 1, PU.REPLACE), 1, KW))
        truth.append(T)
        plain = _px(rng, W + 5, H + 3, 4, 8)
        files.append(oracle.encode(plain, **KW))
        truth.append(plain)
    from pdn_jpegxl_amd.synth import synth
    files.append(oracle.encode(synth(200, 150, 3), distance=1.0))
    truth.append(None)
    lay = LU.layered(oracle.encode(np.zeros((40, 50, 4), np.uint8), **KW),
                     [LU.Layer(oracle.encode(_px(rng, 50, 40, 4, 8), **KW), crop=False), LU.Layer(oracle.encode(_px(rng, 20, 20, 4, 8), **KW), x0=5, y0=5)])
    files.append(lay)
    truth.append(None)
    shapes = [(api.peek(f).height, api.peek(f).width, api.peek(f).num_channels) for f in files]
    outs = [torch.zeros(int(np.prod(s)), dtype=torch.uint8, device="cuda") for s in shapes]
    torch.cuda.synchronize()
    st = gpu_decoder.decode_batch(files, [o.data_ptr() for o in outs], raise_on_error=False)
    assert list(st) == [0] * len(files), (st, gpu_decoder.last_error)
    got = [o.cpu().numpy().reshape(s) for o, s in zip(outs, shapes)]
    for k, t in enumerate(truth):
        alone = api.load_image(files[k]).pixels
        assert (got[k] == alone).all(), k
        if t is not None:
            assert (got[k] == t).all(), k
    # band decode: refused for the patched file only
    out = torch.zeros(int(np.prod(shapes[0])), dtype=torch.uint8, device="cuda")
    gpu_decoder.set_option("band_first_row", 0)
    gpu_decoder.set_option("band_rows", 1)
    try:
        st = gpu_decoder.decode_batch([files[0]], [out.data_ptr()], raise_on_error=False)
        assert st[0] != 0 and "band decode of an image with patches is not supported" in gpu_decoder.last_error, gpu_decoder.last_error
    finally:
        gpu_decoder.set_option("band_rows", 0)
