"""Layered stills, host side (no GPU): the test-stream builder and the parser's acceptance / refusal of layered files."""
import numpy as np
import pytest

import layer_util as LU
from pdn_jpegxl_amd import api


def _img(rng, w, h, c=4):
    return rng.integers(0, 256, (h, w, c), dtype=np.uint8)


@pytest.fixture(scope="module")
def parts(oracle):
    rng = np.random.default_rng(5)
    P = {}
    P["canvas"] = oracle.encode(_img(rng, 100, 80), lossless=True, container=False)
    P["full"] = oracle.encode(_img(rng, 100, 80), lossless=True, container=False)
    P["small"] = oracle.encode(_img(rng, 30, 20), lossless=True, container=False)
    P["lossy_canvas"] = oracle.encode(_img(rng, 100, 80), distance=1.0, container=False)
    P["lossy_small"] = oracle.encode(_img(rng, 30, 20), distance=1.0, container=False)
    return P


BLEND = [LU.Blending(2, 0, False, 0), LU.Blending(2, 0, False, 0)]


def test_frame_header_reemitted_unchanged_is_bit_identical(oracle, parts):
    for key in ("canvas", "small", "lossy_small"):
        cs = parts[key]
        info, h, end = LU.frame_of(cs)
        assert LU.reemit_frame(cs, h, info, (info.xsize, info.ysize), end) == cs[info.frame_start:]
    # with animation fields (duration) in the header as well
    cs = oracle.encode(np.zeros((20, 24, 4), np.uint8), lossless=True, container=False, animation_frames=2)
    info, h, end = LU.frame_of(cs)
    assert info.have_animation
    assert h.duration > 0 and LU.reemit_frame(cs, h, info, (info.xsize, info.ysize), end) == cs[info.frame_start:]


def test_layered_lossless_parses_and_peeks_as_the_canvas(parts):
    f = LU.layered(parts["canvas"], [LU.Layer(parts["full"], crop=False), LU.Layer(parts["small"], x0=-5, y0=70, blending=BLEND, name=b"top")])
    st, _, msg = api.parse_check(f)
    assert st == "Ok", msg
    info = api.peek(f)
    assert (info.width, info.height, info.num_channels) == (100, 80, 4)


def test_layered_lossy_replace_parses(parts):
    """Lossy (XYB) frames are accepted in layered images whose frames all replace (kReplace, with or without a crop)."""
    f = LU.layered(parts["lossy_canvas"], [LU.Layer(parts["lossy_canvas"], crop=False), LU.Layer(parts["lossy_small"], x0=-3, y0=70)])
    st, _, msg = api.parse_check(f)
    assert st == "Ok", msg
    assert (api.peek(f).width, api.peek(f).height) == (100, 80)


def test_lone_frame_blending_its_alpha_is_layered(parts):
    """A lone full-canvas frame whose alpha channel multiplies onto the empty canvas is composited (alpha 0 by the rules), not taken
    for a single-frame image: the host reports the layered image's facts (no MA tree of its own: facts[0] == 0)."""
    plain = LU.layered(parts["canvas"], [LU.Layer(parts["full"], crop=False)])
    mul = LU.layered(parts["canvas"], [LU.Layer(parts["full"], crop=False, blending=[LU.Blending(0, 0, False, 0), LU.Blending(4, 0, False, 0)])])
    assert api.parse_check(plain)[0] == "Ok" and api.parse_check(plain)[1][0] > 0
    assert api.parse_check(mul)[0] == "Ok" and api.parse_check(mul)[1][0] == 0


def test_single_cropped_frame_is_a_layered_image(parts):
    """One frame with a crop is composited onto an empty canvas: accepted, and peek reports the canvas, not the crop."""
    f = LU.layered(parts["canvas"], [LU.Layer(parts["small"], x0=10, y0=10)])
    assert api.parse_check(f)[0] == "Ok"
    assert (api.peek(f).width, api.peek(f).height) == (100, 80)


@pytest.mark.parametrize("case,needle", [
    ("reference_only", "reference-only frames are not supported yet (layered image, frame 0)"),
    ("upsampled", "upsampled frames are not supported yet (layered image, frame 0)"),
    ("lossy_blend", "blend modes other than replace on lossy (XYB) frames are not supported"),
    ("lossy_save_before_ct", "save_before_ct on lossy (XYB) frames is not supported"),
    ("patches", "patches are not supported yet (layered image, frame 0)"),
    ("lf_frame", "LF frames are not supported yet (layered image, frame 0)"),
    ("too_many", "frames before the displayed one are not supported"),
    ("blend_without_alpha", "weighted by a channel other than the alpha channel"),
])
def test_refused_layered_files_name_the_feature(oracle, parts, case, needle):
    c, full, small = parts["canvas"], parts["full"], parts["small"]
    if case == "reference_only":
        f = LU.layered(c, [LU.Layer(full, crop=False, frame_type=2), LU.Layer(small, x0=3, y0=4)])
    elif case == "upsampled":
        f = LU.layered(c, [LU.Layer(full, crop=False, upsampling2=True), LU.Layer(small, x0=3, y0=4)])
    elif case == "lossy_blend":
        f = LU.layered(parts["lossy_canvas"], [LU.Layer(parts["lossy_small"], x0=3, y0=4, blending=BLEND)])
    elif case == "lossy_save_before_ct":
        f = LU.layered(parts["lossy_canvas"], [LU.Layer(parts["lossy_canvas"], crop=False, save_before_ct=True), LU.Layer(parts["lossy_small"], x0=3, y0=4)])
    elif case == "patches":
        f = LU.layered(c, [LU.Layer(full, crop=False, flags=2), LU.Layer(small, x0=3, y0=4)])
    elif case == "lf_frame":
        f = LU.layered(c, [LU.Layer(full, crop=False, flags=32), LU.Layer(small, x0=3, y0=4)])
    elif case == "too_many":
        f = LU.layered(c, [LU.Layer(small, x0=k, y0=k) for k in range(65)])
    else:
        rgb = oracle.encode(np.zeros((20, 30, 3), np.uint8), lossless=True, container=False)
        rgbc = oracle.encode(np.zeros((80, 100, 3), np.uint8), lossless=True, container=False)
        f = LU.layered(rgbc, [LU.Layer(rgbc, crop=False), LU.Layer(rgb, x0=3, y0=4, blending=[LU.Blending(2, 0, False, 0)])])
    st, _, msg = api.parse_check(f)
    assert st == "DecodeError" and needle in msg, (st, msg)
