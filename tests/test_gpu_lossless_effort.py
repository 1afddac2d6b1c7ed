"""GPU tests of the lossless efforts 8 and 9 (DESIGN.md §2 "Lossless efforts 8 and 9", §4.11): palette, reversible colour transform
and predictor search (8), the weighted predictor's state and property-15 contexts (9), the fallback to effort 7.  The ground truth of
every round trip is the source picture, read back by the product's decoder and by the CPU oracle."""
import numpy as np
import pytest

from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth

pytestmark = pytest.mark.gpu


def bgra_of(rgba):
    return np.ascontiguousarray(rgba[..., [2, 1, 0, 3]])


def layout_of(img, layout):
    """An RGBA source whose analysis (all gray? all opaque?) gives the wanted coded channels, and those channels."""
    img = img.copy()
    if layout in ("gray", "gray+alpha"):
        img[..., 0] = img[..., 2] = img[..., 1]
    if layout in ("rgb", "gray"):
        img[..., 3] = 255
    else:
        img[0, 0, 3] = 7            # some pixel is not opaque, whatever the picture
    if layout in ("rgba", "rgb") and img.shape[0] * img.shape[1] > 0:
        img[0, 0, 0] = img[0, 0, 1] ^ 0x40   # some pixel is not gray
    want = {"rgba": img, "rgb": img[..., :3], "gray": img[..., 1:2], "gray+alpha": img[..., [1, 3]]}[layout]
    return img, np.ascontiguousarray(want)


def save(img, effort):
    data = api.save_image(bgra_of(img), lossless=True, effort=effort)
    return data, api.last_save_lossless_info()


def check_round_trip(oracle, data, want):
    got = api.load_image(data).pixels
    assert got.shape == want.shape and (got == want).all()
    ref = oracle.decode(data).pixels
    assert ref.shape == want.shape and (ref == want).all()


# ------------------------------------------------------------------ 1. round trip
# 1x1 .. 3x2: the NW / NE clamps and widths below the skew; 1x70, 70x1, 2x130: more than one 64-row band at minimal width, two bands and
# a remainder; 257x3, 3x257, 258x259: a column / row past the group edge, four groups with 2- and 3-pixel edge groups; 130x90 and
# 300x280: the ordinary one-group and four-group cases.
SIZES = [(1, 1), (2, 1), (1, 2), (3, 2), (1, 70), (70, 1), (2, 130), (257, 3), (3, 257), (258, 259), (130, 90), (300, 280)]


@pytest.mark.parametrize("layout", ["rgba", "rgb", "gray", "gray+alpha"])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("effort", [8, 9])
def test_round_trip_is_bit_exact(oracle, effort, size, layout):
    w, h = size
    img, want = layout_of(synth(w, h, 3 + w + h), layout)
    data, info = save(img, effort)
    assert info["tier"] == effort
    check_round_trip(oracle, data, want)


# ------------------------------------------------------------------ 2. palette
def palette_image(w, h, ncol, nch, seed):
    """Flat regions of ncol distinct colours over nch channels (1..4: Gray, GrayA, RGB, RGBA), as an RGBA source."""
    rng = np.random.default_rng(seed)
    cols = np.zeros((0, nch), np.uint8)
    while len(cols) < ncol:   # distinct colours
        cols = np.unique(np.concatenate([cols, rng.integers(0, 256, (ncol, nch), dtype=np.uint8)]), axis=0)
    cols = cols[rng.permutation(len(cols))[:ncol]]
    if nch in (2, 4):
        cols[0, -1] = 9        # not opaque
    if nch >= 3:
        cols[0, 0] = cols[0, 1] ^ 0x40   # not gray
    yy, xx = np.mgrid[0:h, 0:w]
    idx = (xx // 7 + yy // 5 + (xx * yy) // 977) % ncol
    if w * h >= ncol:
        idx.reshape(-1)[:ncol] = np.arange(ncol)   # every colour occurs
    px = cols[idx]
    rgba = np.full((h, w, 4), 255, np.uint8)
    if nch <= 2:
        rgba[..., :3] = px[..., :1]
    else:
        rgba[..., :3] = px[..., :3]
    if nch in (2, 4):
        rgba[..., 3] = px[..., -1]
    return rgba, np.ascontiguousarray(px)


PALETTES = {"5 colours gray+alpha": (120, 90, 5, 2), "5 colours rgba": (120, 90, 5, 4), "17 colours rgba": (300, 200, 17, 4),
            "1024 colours rgb": (258, 259, 1024, 3), "1025 colours rgb": (258, 259, 1025, 3)}


@pytest.mark.parametrize("name", list(PALETTES))
def test_palette(oracle, name):
    w, h, ncol, nch = PALETTES[name]
    img, want = palette_image(w, h, ncol, nch, 7 * ncol + nch)
    assert len(np.unique(want.reshape(-1, nch), axis=0)) == ncol
    size = {}
    for effort in (7, 8, 9):
        data, info = save(img, effort)
        size[effort] = len(data)
        check_round_trip(oracle, data, want)
        if effort >= 8:
            assert info["palette_colours"] == (ncol if ncol <= 1024 else 0), info
            if ncol <= 1024:
                assert len(info["predictors"]) == 1 and info["rct_type"] == -1
    print("%s: effort 7 / 8 / 9 = %d / %d / %d bytes" % (name, size[7], size[8], size[9]))
    if ncol <= 17:
        assert size[8] < size[7] / 2, size


# ------------------------------------------------------------------ 3. colour transform
def independent_channels(w, h):
    img = np.stack([synth(w, h, 11)[..., 1], synth(w, h, 12)[..., 1], synth(w, h, 13)[..., 1], np.full((h, w), 255, np.uint8)], axis=-1)
    return np.ascontiguousarray(img)


def test_colour_transform_is_searched(oracle):
    img = independent_channels(264, 200)
    d7, _ = save(img, 7)
    d8, info = save(img, 8)
    print("independent channels 264x200: effort 7 / 8 = %d / %d bytes, %s" % (len(d7), len(d8), info))
    check_round_trip(oracle, d8, img[..., :3])
    assert info["rct_type"] != 6 and 0 <= info["rct_type"] < 6
    assert len(d8) <= 0.965 * len(d7), (len(d8), len(d7))


def test_info_reports_transform_and_predictors(oracle):
    img = synth(264, 200, 5)
    data, info = save(img, 8)
    print("synth(264,200,5) effort 8: %s" % info)
    check_round_trip(oracle, data, img)
    assert info["tier"] == 8 and info["palette_colours"] == 0 and 0 <= info["rct_type"] <= 6
    assert len(info["predictors"]) == 4 and all(1 <= p <= 5 for p in info["predictors"])
    assert info["leaves"] == 4 and 1 <= info["clusters"] <= 4
    assert info["searched_bytes"] > 0 and info["effort7_bytes"] > 0
    names = list(api.last_save_stage_times())
    for stage in ("colour count", "transform and predictor search", "tokens", "sections"):
        assert any(stage in n for n in names), names


# ------------------------------------------------------------------ 4. contexts and weighted predictor
PHOTOS = {"264x200": (264, 200, 5), "300x280": (300, 280, 3), "512x384": (512, 384, 7)}


@pytest.mark.parametrize("name", list(PHOTOS))
def test_weighted_predictor_and_contexts_pay(oracle, name):
    w, h, seed = PHOTOS[name]
    img = synth(w, h, seed)
    size, infos = {}, {}
    for effort in (7, 8, 9):
        data, infos[effort] = save(img, effort)
        size[effort] = len(data)
        if effort == 9:
            check_round_trip(oracle, data, img)
            names = list(api.last_save_stage_times())
            assert any("weighted pass" in n for n in names), names
    theirs = len(oracle.encode(img, lossless=True))
    print("synth(%d,%d,%d): effort 7 / 8 / 9 = %d / %d / %d bytes, the oracle's default stream %d; effort 9: %s"
          % (w, h, seed, size[7], size[8], size[9], theirs, infos[9]))
    assert size[9] <= size[8] <= size[7], size
    assert size[9] <= 0.945 * size[7], size
    assert infos[9]["tier"] == 9 and not infos[9]["fell_back_to_effort7"]


# ------------------------------------------------------------------ 5. fallback
def test_never_larger_than_effort_7_on_noise(oracle):
    img = np.random.default_rng(5).integers(0, 256, (90, 130, 4), dtype=np.uint8)
    d7, _ = save(img, 7)
    for effort in (8, 9):
        data, info = save(img, effort)
        print("noise 130x90 effort %d: %d bytes (effort 7: %d), %s" % (effort, len(data), len(d7), info))
        assert len(data) <= len(d7)
        if info["fell_back_to_effort7"]:
            assert data == d7
        else:
            assert len(data) < len(d7)
        check_round_trip(oracle, data, img)


def test_fallback_writes_the_bytes_of_effort_7():
    """A picture the search cannot shrink: one pixel.  (Whatever it is on other pictures, the flag and the bytes agree.)"""
    for img in (np.full((1, 1, 4), 90, np.uint8), synth(3, 2, 1)):
        d7, _ = save(img, 7)
        for effort in (8, 9):
            data, info = save(img, effort)
            assert info["fell_back_to_effort7"] == (info["searched_bytes"] >= info["effort7_bytes"])
            assert (data == d7) == info["fell_back_to_effort7"] and len(data) <= len(d7)


# ------------------------------------------------------------------ 6. determinism and unchanged ground
def test_same_input_same_bytes():
    pal, _ = palette_image(300, 200, 17, 4, 123)
    for img in (pal, synth(264, 200, 5)):
        assert save(img, 9)[0] == save(img, 9)[0]


def test_lower_efforts_and_lossy_saves_report_tier_0():
    img = synth(130, 90, 2)
    _, info = save(img, 9)
    assert info["tier"] == 9
    _, info = save(img, 7)
    assert info["tier"] == 0 and info["palette_colours"] == 0 and info["predictors"] == [] and info["searched_bytes"] == 0
    save(img, 9)
    api.save_image(bgra_of(img), distance=1.0, effort=9)
    assert api.last_save_distances()["evaluations"] == 5        # the lossy side still runs its quantisation loop
    assert api.last_save_lossless_info()["tier"] == 0


def test_progress_is_monotone_and_a_cancel_is_honoured():
    bgra = bgra_of(synth(264, 200, 5))
    seen = []
    api.save_image(bgra, lossless=True, effort=9, progress=lambda p: seen.append(p) or True)
    assert seen == sorted(seen) and seen[0] == 0 and seen[-1] == 95 and {0, 5, 15, 30, 90, 95} <= set(seen)
    before_output = sum(p < 30 for p in seen)
    assert before_output >= 6       # checkpoints between the stages of the search
    for stop_at in range(3, before_output + 1):
        calls = []
        with pytest.raises(api.JxlError) as e:
            api.save_image(bgra, lossless=True, effort=9, progress=lambda p: calls.append(p) or len(calls) < stop_at)
        assert e.value.status == "UserCanceled" and len(calls) == stop_at and calls == sorted(calls)
        assert api.last_save_lossless_info()["tier"] == 0
