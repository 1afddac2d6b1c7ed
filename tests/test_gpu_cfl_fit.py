"""GPU tests of the chroma-from-luma fit of the lossy encoder (JxlHipLossyOptions::chroma_from_luma, DESIGN.md §2 "Chroma from luma,
fitted"): jxlhip_save_pixels_lossy / jxlhip_encode_batch_lossy against the calls without the struct, the fitted maps against the
oracle's fit of the same pixels, round trips on both decoders, the bytes saved, the shapes where the fit or its coding can go wrong,
deep samples, the batch, the refusals.  What these rest on is shown on the oracle alone in test_cfl_fit_host.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import cfl_util as U
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth
from save_pixels_util import float_image, nominal, psnr_nominal, u16_image

pytestmark = pytest.mark.gpu


def device_item(px, **kw):
    host = np.array(px, order="C")   # (a writable copy: the pictures of cfl_util are read-only)
    h, w, c = host.shape
    dev = torch.from_numpy(host.view(np.uint8).reshape(h, -1)).cuda()
    return api.EncodeItem(dev.data_ptr(), w, h, c, px.dtype, keep=dev, **kw)


@pytest.fixture(scope="module")
def encoder():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the product path has no CPU fallback")
    enc = api.Encoder(0)
    yield enc
    enc.close()


def both_decoders_agree(oracle, data, bound=1):
    """The product's decode of `data` against the oracle's; returns the oracle's."""
    od = oracle.decode(data)
    got = api.load_image(data)
    assert got.pixels.shape == od.pixels.shape
    assert np.abs(got.pixels.astype(int) - od.pixels.astype(int)).max() <= bound
    return od


# ---------------------------------------------------------------- 1. off is the old file
def off_cases():
    rgba = synth(300, 280, 3)
    return {
        "rgb": (np.ascontiguousarray(rgba[..., :3]), dict(distance=1.0, effort=7)),
        "rgba": (rgba, dict(distance=2.0, effort=5)),
        "u16": (u16_image(264, 200, 5, 12, 4), dict(bits=12, distance=1.0, effort=7)),
        "f32": (float_image(264, 200, 7, np.float32, 3), dict(distance=1.0, effort=3, colour="LinearSrgb")),
        "lossless": (np.ascontiguousarray(rgba[:100, :120, :3]), dict(lossless=True, effort=7)),
    }


@pytest.mark.parametrize("name", list(off_cases()))
def test_off_through_the_new_call_is_the_file_of_save_pixels(name):
    px, kw = off_cases()[name]
    old = api.save_pixels(px, cfl=None, **kw)        # jxlhip_save_pixels
    assert api.save_pixels(px, cfl=False, **kw) == old
    if kw.get("lossless"):
        assert api.save_pixels(px, cfl=True, **kw) == old   # a lossless save ignores the struct


def test_off_through_the_new_batch_call_is_the_file_of_encode_batch(encoder):
    cases = off_cases()
    items = [device_item(px, **kw) for px, kw in cases.values()]
    old = encoder.encode_batch(items, lossy_call=False)   # jxlhip_encode_batch
    assert all(f is not None for f in old)
    assert encoder.encode_batch(items, lossy_call="null") == old
    assert encoder.encode_batch(items, lossy_call=True) == old
    assert old == [api.save_pixels(px, cfl=None, **kw) for px, kw in cases.values()]


# ---------------------------------------------------------------- 2. the maps against the oracle's fit
# Tiles (of both maps together) whose value differs from the oracle's, measured on the first run on an MI355X: (picture, effort) ->
# (differing, compared).  The oracle sums in double and this kernel in float, and a Y coefficient that quantises the other way moves
# the sums, so a value near a rounding boundary may land on the other side: by one at the most.
MEASURED_DIFFERING = {("synth", 3): (0, 96), ("synth", 5): (0, 96), ("synth", 7): (0, 96), ("tex", 3): (0, 12), ("tex", 5): (0, 12), ("tex", 7): (0, 12),
                      ("wide", 3): (0, 132)}
PICTURES = {"synth": ("synth", 512, 384, 7), "tex": ("tex", 192, 128, 3), "wide": ("synth", 2112, 72, 11)}


def compare_maps(oracle, name, effort, mode):
    pic = PICTURES[name]
    img = U._PICTURES[pic[0]](*pic[1:])
    ours = oracle.decode(api.save_pixels(img, distance=1.0, effort=effort, cfl=True), want_dump=True)
    theirs = U.oracle_dump(*pic, 1.0, mode)
    (ox, ob), (tx, tb) = U.maps_of(ours), U.maps_of(theirs)
    assert ox.any() or ob.any()                         # (the encoder without the fit writes maps that are all zero)
    ok = U.tiles_that_agree(ours, theirs)
    if effort == 3:
        assert (ours.planes["strategy"] == theirs.planes["strategy"]).all()
        ok[:] = True                                    # 8x8 DCTs only, the same by construction: every tile is compared
    assert ok.mean() >= 0.5
    dx, db = np.abs(ox - tx)[ok], np.abs(ob - tb)[ok]
    differing, compared = int((dx > 0).sum() + (db > 0).sum()), 2 * int(ok.sum())
    print("%s effort %d: %d of %d tiles compared, %d of %d map values differ from the oracle's, max |delta| %d" %
          (name, effort, int(ok.sum()), ok.size, differing, compared, max(dx.max(), db.max())))
    assert dx.max() <= 1 and db.max() <= 1
    measured, of = MEASURED_DIFFERING[(name, effort)]
    assert differing <= max(3, int(np.ceil(2.0 * measured / of * compared)))
    return ox, ob


@pytest.mark.parametrize("effort,mode", U.EFFORTS, ids=["fast", "squares", "default"])
@pytest.mark.parametrize("name", ["synth", "tex"])
def test_fitted_maps_match_the_oracles_fit(oracle, name, effort, mode):
    ox, ob = compare_maps(oracle, name, effort, mode)
    if name == "tex":
        assert (ob == -128).all()                       # clamped in every tile (test_cfl_fit_host.py)


# ---------------------------------------------------------------- 3. round trip
def round_trip(oracle, img, effort, mode, distance=1.0):
    """Fitting on: both decoders agree, alpha exact, PSNR against the oracle's fitted file and our own file without fitting."""
    on = api.save_pixels(img, distance=distance, effort=effort, cfl=True)
    od = both_decoders_agree(oracle, on)
    if img.shape[2] == 4:
        assert (od.pixels[..., 3] == img[..., 3]).all()
        assert (api.load_image(on).pixels[..., 3] == img[..., 3]).all()
    ours = U.psnr(od.pixels[..., :3], img[..., :3])
    theirs = U.psnr(oracle.decode(oracle.encode(img, distance=distance, strategy_mode=mode, side_info=dict(cfl="fitted"))).pixels[..., :3], img[..., :3])
    off = api.save_pixels(img, distance=distance, effort=effort, cfl=False)
    ours_off = U.psnr(oracle.decode(off).pixels[..., :3], img[..., :3])
    print("effort %d: PSNR %.3f dB, the oracle's fitted file %.3f dB, our file without fitting %.3f dB; %d bytes against %d" %
          (effort, ours, theirs, ours_off, len(on), len(off)))
    assert ours > theirs - 0.5
    assert ours >= ours_off - 0.1
    return on, off


@pytest.mark.parametrize("effort,mode", U.EFFORTS, ids=["fast", "squares", "default"])
@pytest.mark.parametrize("name", ["rgba300x280", "tex65x130"])
def test_round_trip(oracle, name, effort, mode):
    img = synth(300, 280, 3) if name == "rgba300x280" else U.colour_tex(65, 130, 5)
    round_trip(oracle, img, effort, mode)


def test_round_trip_through_the_closed_loop(oracle):
    img = U.synth_rgb(256, 192, 7)
    round_trip(oracle, img, 8, 0)
    api.save_pixels(img, distance=1.0, effort=8, cfl=True)
    assert api.last_save_distances()["evaluations"] == 3


# ---------------------------------------------------------------- 4. bytes
@pytest.mark.parametrize("pic,bound", [(("tex", 192, 128, 3), 0.80), (("tex", 65, 130, 5), 0.85), (("synth", 512, 384, 7), 0.99)],
                         ids=["tex192x128", "tex65x130", "synth512x384"])
def test_fitting_saves_bytes(pic, bound):
    img = U._PICTURES[pic[0]](*pic[1:])
    on, off = (len(api.save_pixels(img, distance=1.0, effort=7, cfl=c)) for c in (True, False))
    print("bytes on / off = %d / %d = %.4f" % (on, off, on / off))
    assert on / off <= bound


# ---------------------------------------------------------------- 5. shapes where it can go wrong
def test_partial_tiles_on_both_edges(oracle):
    img = U.colour_tex(65, 130, 5)
    d = oracle.decode(api.save_pixels(img, distance=3.0, effort=7, cfl=True), want_dump=True)
    ytox, ytob = U.maps_of(d)
    assert ytox.shape == (3, 2) and ytox.any() and ytob.any()
    both_decoders_agree(oracle, api.save_pixels(img, distance=3.0, effort=7, cfl=True))


def test_second_lf_group_of_one_tile_column(oracle):
    ox, ob = compare_maps(oracle, "wide", 3, 1)
    assert ox.shape == (2, 33) and ox[:, 32].any() and ob[:, 32].any()
    both = np.concatenate([ox.ravel(), ob.ravel()])
    assert both.min() == -128 and both.max() == 127     # both clamps
    both_decoders_agree(oracle, api.save_pixels(U.synth_rgb(2112, 72, 11), distance=1.0, effort=3, cfl=True))


@pytest.mark.parametrize("size", [(8, 8), (1, 1)], ids=["8x8", "1x1"])
@pytest.mark.parametrize("effort", [3, 7])
def test_tiny_frames(oracle, size, effort):
    both_decoders_agree(oracle, api.save_pixels(U.colour_tex(size[0], size[1], 2), distance=1.0, effort=effort, cfl=True))


@pytest.mark.parametrize("name", ["flat64", "1x1"])
def test_all_zero_maps_write_the_off_file(oracle, name):
    img = U.flat64() if name == "flat64" else U.colour_tex(1, 1, 2)
    on = api.save_pixels(img, distance=1.0, effort=7, cfl=True)
    assert on == api.save_pixels(img, distance=1.0, effort=7, cfl=False)
    both_decoders_agree(oracle, on)


def test_one_group_rgba_frame_shares_the_modular_code_with_its_alpha(oracle):
    img = synth(200, 120, 19)
    on = api.save_pixels(img, distance=1.0, effort=7, cfl=True)
    od = both_decoders_agree(oracle, on)
    assert (od.pixels[..., 3] == img[..., 3]).all()
    ytox, ytob = U.maps_of(oracle.decode(on, want_dump=True))
    assert ytox.any() or ytob.any()


# ---------------------------------------------------------------- 6. deep samples
@pytest.mark.parametrize("kind", ["u12", "f32"])
def test_deep_samples_round_trip(oracle, kind):
    """As test_round_trip; the two decoders agree within what tests/test_gpu_save_pixels.py allows for the sample type."""
    if kind == "u12":
        px, kw, okw, bits = u16_image(300, 280, 3, 12, 4), dict(bits=12), dict(bits=12), 12
    else:
        px, kw, okw, bits = float_image(300, 280, 3, np.float32, 4), dict(), dict(float_samples=32), None
    on = api.save_pixels(px, distance=1.0, effort=7, cfl=True, **kw)
    od = oracle.decode(on).pixels
    got = api.load_image(on).pixels
    assert od.shape == px.shape and got.shape == od.shape and got.dtype == od.dtype
    if kind == "u12":
        d = np.abs(got.astype(np.int32) - od.astype(np.int32))
        assert d[..., :3].max() <= 48 and d[..., 3].max() == 0
    else:
        assert np.abs(got[..., :3] - od[..., :3]).max() < 1e-3
        assert np.array_equal(od[..., 3].view(np.uint32), px[..., 3].view(np.uint32))
    assert np.any(U.maps_of(oracle.decode(on, want_dump=True))[0])
    src = nominal(px, bits)
    ours = psnr_nominal(nominal(od)[..., :3], src[..., :3])
    ref = oracle.decode(oracle.encode(px, distance=1.0, strategy_mode=0, side_info=dict(cfl="fitted"), **okw)).pixels
    theirs = psnr_nominal(nominal(ref)[..., :3], src[..., :3])
    off = oracle.decode(api.save_pixels(px, distance=1.0, effort=7, cfl=False, **kw)).pixels
    ours_off = psnr_nominal(nominal(off)[..., :3], src[..., :3])
    print("%s: PSNR %.3f dB, the oracle's fitted file %.3f dB, our file without fitting %.3f dB" % (kind, ours, theirs, ours_off))
    assert ours > theirs - 0.5 and ours >= ours_off - 0.1


# ---------------------------------------------------------------- 7. batch
def test_batch_writes_the_bytes_of_the_single_call_run_after_run(encoder):
    rgba = synth(300, 280, 3)
    cases = [(U.colour_tex(192, 128, 3), dict(distance=1.0, effort=7, cfl=True)),
             (U.synth_rgb(256, 192, 7), dict(distance=1.0, effort=7, cfl=False)),
             (np.ascontiguousarray(rgba[:100, :120, :3]), dict(lossless=True, effort=7, cfl=True)),
             (rgba, dict(distance=2.0, effort=5, cfl=True)),
             (U.synth_rgb(2112, 72, 11), dict(distance=1.0, effort=3, cfl=True))]
    items = [device_item(px, **kw) for px, kw in cases]
    want = [api.save_pixels(px, **kw) for px, kw in cases]
    first = encoder.encode_batch(items)
    assert first == want
    assert encoder.encode_batch(items) == want
    assert encoder.encode_batch(items[::-1]) == want[::-1]


# ---------------------------------------------------------------- 8. refusals
BAD = {"2": (2, (0, 0, 0)), "-1": (-1, (0, 0, 0)), "reserved": (1, (0, 7, 0))}


@pytest.mark.parametrize("name", list(BAD))
def test_save_refuses_a_bad_struct_before_any_write(name):
    v, reserved = BAD[name]
    img = U.synth_rgb(256, 192, 7)
    writes = []
    L = api.lib()
    desc = api.JxlHipPixels(img.ctypes.data, 256, 192, 256 * 3, 3, 0, 8, api.KNOWN_PROFILE.index("Srgb"))
    io = api.IOCallbacks(api.WriteFn(lambda p, n: writes.append(n) or api.S_OK), api.SeekFn(lambda p: api.S_OK))
    err = api.ErrorInfo()
    lossy = api.JxlHipLossyOptions(v, (C.c_int32 * 3)(*reserved))
    st = L.jxlhip_save_pixels_lossy(C.byref(desc), C.byref(api.EncoderOptions(1.0, 7, False)), C.byref(lossy), C.byref(api.EncoderImageMetadata()),
                                    C.byref(io), C.byref(err), api.ProgressFn())
    assert api.ENCODER_STATUS[st] == "EncodeError" and "JxlHipLossyOptions" in err.errorMessage.decode() and not writes
    with pytest.raises(api.JxlError) as e:
        api.save_pixels(img, cfl=lossy)
    assert e.value.status == "EncodeError"
    assert api.save_pixels(img, cfl=True) == api.save_pixels(img, cfl=api.JxlHipLossyOptions(1))   # usable afterwards


@pytest.mark.parametrize("name", list(BAD))
def test_batch_refuses_a_bad_struct_per_image(encoder, name):
    v, reserved = BAD[name]
    img = U.synth_rgb(256, 192, 7)
    good = device_item(img, cfl=True)
    bad = device_item(img, cfl=api.JxlHipLossyOptions(v, (C.c_int32 * 3)(*reserved)))
    out = encoder.encode_batch([good, bad], raise_on_error=False)
    assert encoder.last_statuses == ["Ok", "EncodeError"] and out[1] is None
    assert encoder.last_error.startswith("image 1:") and "JxlHipLossyOptions" in encoder.last_error
    want = api.save_pixels(img, cfl=True)
    assert out[0] == want
    assert encoder.encode_batch([good]) == [want]
