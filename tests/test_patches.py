"""Patches, host side (no GPU): the dictionary parser and the layered walk's rules for reference-only frames and patches."""
import numpy as np
import pytest

import layer_util as LU
import patch_util as PU
from pdn_jpegxl_amd import api

W, H = 100, 80
R, A, N = (PU.REPLACE, 0, False), (PU.ADD, 0, False), (PU.NONE, 0, False)


@pytest.fixture(scope="module")
def parts(oracle):
    rng = np.random.default_rng(31)
    kw = dict(lossless=True, container=False)
    img = lambda w, h, c=4: rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    P = {}
    P["canvas"] = oracle.encode(img(W, H), **kw)
    P["frame"] = oracle.encode(img(W, H), **kw)
    P["atlas"] = oracle.encode(img(30, 20), **kw)
    P["big"] = oracle.encode(img(600, 520), **kw)        # several groups: section 0 is LfGlobal alone
    P["big_canvas"] = oracle.encode(img(600, 520), **kw)
    P["rgb_canvas"] = oracle.encode(img(W, H, 3), **kw)
    P["rgb_frame"] = oracle.encode(img(W, H, 3), **kw)
    P["rgb_atlas"] = oracle.encode(img(30, 20, 3), **kw)
    P["lossy_canvas"] = oracle.encode(img(W, H), distance=1.0, container=False)
    P["lossy_atlas"] = oracle.encode(img(30, 20), distance=1.0, container=False)
    return P


def one(parts, refs, nec=1, frame="frame", canvas="canvas", atlas="atlas", **kw):
    """A file of one atlas in slot 0 and one full-canvas frame with the dictionary of `refs`."""
    pf = PU.patched(parts[frame], refs, nec, **kw)
    return LU.layered(parts[canvas], [LU.Layer(parts[atlas], frame_type=2, save_before_ct=True), LU.Layer(pf, crop=False, flags=2)])


def test_token_writer_matches_the_parser(parts):
    """Dictionaries with one and several sections per frame, negative deltas, every blend record shape: accepted, and peek reports
    the canvas."""
    places = [PU.Place(60, 40, [R, R]), PU.Place(10, 50, [A, (PU.BLEND_ABOVE, 0, True)]), PU.Place(0, 0, [(PU.MUL, 0, True), N]),
              PU.Place(95, 74, [(PU.AWADD_BELOW, 0, False), (PU.BLEND_BELOW, 0, False)])]
    f = one(parts, [PU.Ref(0, 2, 3, 5, 6, places), PU.Ref(0, 0, 0, 1, 1, [PU.Place(99, 79, [R, R])])])
    st, _, msg = api.parse_check(f)
    assert st == "Ok", msg
    assert (api.peek(f).width, api.peek(f).height) == (W, H)
    pf = PU.patched(parts["big"], [PU.Ref(0, 0, 0, 30, 20, [PU.Place(570, 500, [R, R]), PU.Place(3, 1, [R, R])])], 1)
    f = LU.layered(parts["big_canvas"], [LU.Layer(parts["atlas"], frame_type=2), LU.Layer(pf, crop=False, flags=2)])
    assert api.parse_check(f)[0] == "Ok", api.parse_check(f)


@pytest.mark.parametrize("case,needle", [
    ("too_many_refs", "patch dictionary: too many reference patches"),
    ("too_many_positions", "patch dictionary: too many patch positions"),
    ("slot_out_of_range", "patch dictionary: reference slot out of range"),
    ("rect_outside_atlas", "patch dictionary: a patch rectangle outside its reference frame (layered image, frame 1)"),
    ("rect_huge", "patch dictionary: a patch rectangle outside its reference frame"),
    ("position_right_edge", "patch dictionary: a patch position outside the frame"),
    ("position_bottom_edge", "patch dictionary: a patch position outside the frame"),
    ("negative_delta", "patch dictionary: a patch position outside the frame"),
    ("blend_mode_8", "patch dictionary: blend mode out of range"),
    ("alpha_without_alpha", "patch blend modes weighted by a channel other than the alpha channel are not supported"),
    ("ans_final_state", "patch dictionary: ANS final state"),
    ("more_positions_than_coded", "patch dictionary: "),
    ("empty_slot", "patches from an empty reference slot (layered image, frame 1)"),
])
def test_dictionary_limits_and_ranges(parts, case, needle):
    ref = lambda places, **k: PU.Ref(k.get("slot", 0), k.get("x0", 0), k.get("y0", 0), k.get("w", 5), k.get("h", 5), places)
    P = PU.Place
    kw = {}
    if case == "too_many_refs":   # 1024 + W * H / 4 is the limit; the count comes first, nothing else is read
        f = LU.layered(parts["canvas"], [LU.Layer(parts["atlas"], frame_type=2), LU.Layer(
            PU.with_dictionary(parts["frame"], *PU.write_tokens([(PU.NUM_REF, 1024 + W * H // 4 + 1)])), crop=False, flags=2)])
    elif case == "too_many_positions":
        toks = [(PU.NUM_REF, 1), (PU.REF_FRAME, 0), (PU.REF_POS, 0), (PU.REF_POS, 0), (PU.SIZE, 0), (PU.SIZE, 0),
                (PU.COUNT, 4 * (1024 + W * H // 4))]
        f = LU.layered(parts["canvas"], [LU.Layer(parts["atlas"], frame_type=2), LU.Layer(
            PU.with_dictionary(parts["frame"], *PU.write_tokens(toks)), crop=False, flags=2)])
    elif case == "more_positions_than_coded":   # 5000 positions claimed, one coded: the reader runs on into LfGlobal's own bits
        toks = PU.tokens([ref([P(1, 1, [R, R])])], 1)
        toks[6] = (PU.COUNT, 4999)
        f = LU.layered(parts["canvas"], [LU.Layer(parts["atlas"], frame_type=2), LU.Layer(
            PU.with_dictionary(parts["frame"], *PU.write_tokens(toks)), crop=False, flags=2)])
    else:
        refs = {
            "slot_out_of_range": [ref([P(1, 1, [R, R])], slot=4)],
            "rect_outside_atlas": [ref([P(1, 1, [R, R])], x0=26)],            # the atlas is 30 x 20
            "rect_huge": [ref([P(1, 1, [R, R])], y0=(1 << 31) - 3)],
            "position_right_edge": [ref([P(96, 0, [R, R])])],
            "position_bottom_edge": [ref([P(0, 76, [R, R])])],
            "negative_delta": [ref([P(3, 3, [R, R]), P(0, 0, [R, R])])],
            "blend_mode_8": [ref([P(1, 1, [R, (8, 0, False)])])],
            "ans_final_state": [ref([P(1, 1, [R, R])])],
            "empty_slot": [ref([P(1, 1, [R, R])], slot=2)],
        }.get(case)
        if case == "negative_delta":
            kw["raw_deltas"] = {(0, 1): (PU.pack_signed(-4), 0)}
        if case == "ans_final_state":
            kw["extra_tokens"] = [(PU.MODE, 1), (PU.POS, 7)]
        if case == "alpha_without_alpha":
            f = one(parts, [ref([P(1, 1, [(PU.BLEND_ABOVE, 0, False)])])], nec=0, frame="rgb_frame", canvas="rgb_canvas", atlas="rgb_atlas")
        else:
            f = one(parts, refs, **kw)
    st, _, msg = api.parse_check(f)
    assert st == "DecodeError" and needle in msg, (st, msg)


def test_negative_deltas_within_the_frame_are_accepted(parts):
    places = [PU.Place(90, 70, [R, R]), PU.Place(3, 60, [R, R]), PU.Place(50, 0, [A, A]), PU.Place(0, 1, [R, R])]
    assert api.parse_check(one(parts, [PU.Ref(0, 1, 1, 8, 9, places)]))[0] == "Ok"


@pytest.mark.parametrize("case,needle", [
    ("regular_slot", "patches from a slot that holds a regular frame are not supported (layered image, frame 2)"),
    ("blend_onto_atlas", "frames blending onto a slot that holds a reference-only frame are not supported (layered image, frame 1)"),
    ("lossy", "patches on lossy (VarDCT / XYB) frames are not supported (layered image, frame 1)"),
    ("patched_atlas", "patches on reference-only frames are not supported yet (layered image, frame 1)"),
    ("overwritten_atlas", "reference-only frames are not supported yet (layered image, frame 0)"),
    ("unread_atlas", "reference-only frames are not supported yet (layered image, frame 1): no patch reads it"),
    ("no_atlas", "patches are not supported yet (layered image, frame 1)"),
    ("lone_frame", "noise / patches / splines are not supported yet"),
])
def test_slot_rules(parts, case, needle):
    at = lambda slot=0: LU.Layer(parts["atlas"], frame_type=2, save_ref=slot)
    pf = lambda slot=0, **k: LU.Layer(PU.patched(parts["frame"], [PU.Ref(slot, 0, 0, 4, 4, [PU.Place(5, 5, [R, R])])], 1), flags=2, **k)
    if case == "regular_slot":
        layers = [at(0), LU.Layer(parts["frame"], crop=False, save_ref=1), pf(1, crop=False)]
    elif case == "blend_onto_atlas":   # the patched frame is a crop (it reads its source slot outside the crop): slot 0 holds the atlas
        layers = [at(0), LU.Layer(PU.patched(parts["atlas"], [PU.Ref(0, 0, 0, 4, 4, [PU.Place(5, 5, [R, R])])], 1), x0=3, y0=4, flags=2)]
    elif case == "lossy":
        f = LU.layered(parts["lossy_canvas"], [LU.Layer(parts["lossy_atlas"], frame_type=2),
                                               LU.Layer(parts["lossy_canvas"], crop=False, flags=2)])
    elif case == "patched_atlas":
        layers = [at(0), LU.Layer(parts["atlas"], frame_type=2, save_ref=1, flags=2), pf(0, crop=False)]
    elif case == "overwritten_atlas":   # frame 1 (a regular frame) replaces the atlas in slot 0 before anything could read it
        layers = [at(0), LU.Layer(parts["frame"], crop=False, save_ref=0), LU.Layer(parts["frame"], crop=False)]
    elif case == "unread_atlas":   # a second atlas in slot 1 that the dictionary does not read
        layers = [at(0), at(1), pf(0, crop=False)]
    elif case == "no_atlas":   # the patches flag on frame 1 with only a regular frame in the slots
        layers = [LU.Layer(parts["frame"], crop=False), LU.Layer(parts["frame"], crop=False, flags=2)]
    else:   # one full-canvas frame alone: a single-frame image, which has no reference frame for its patches
        layers = [pf(0, crop=False)]
    if case != "lossy":
        f = LU.layered(parts["canvas"], layers)
    st, _, msg = api.parse_check(f)
    assert st == "DecodeError" and needle in msg, (st, msg)


def test_pinned_refusal_shapes_keep_their_messages(parts):
    """A reference-only frame followed by a plain cropped frame, and the patches flag on frame 0 with no dictionary, are refused as before
    (tests/test_layers.py pins both); so is the first through peek's header-only parse."""
    f = LU.layered(parts["canvas"], [LU.Layer(parts["frame"], crop=False, frame_type=2), LU.Layer(parts["atlas"], x0=3, y0=4)])
    st, _, msg = api.parse_check(f)
    assert st == "DecodeError" and "reference-only frames are not supported yet (layered image, frame 0)" in msg, msg
    with pytest.raises(api.JxlError) as e:
        api.peek(f)
    assert "reference-only frames are not supported yet (layered image, frame 0)" in str(e.value)
    f = LU.layered(parts["canvas"], [LU.Layer(parts["frame"], crop=False, flags=2), LU.Layer(parts["atlas"], x0=3, y0=4)])
    st, _, msg = api.parse_check(f)
    assert st == "DecodeError" and "patches are not supported yet (layered image, frame 0)" in msg, msg


def test_cropped_atlas_and_cropped_patched_layer_parse(parts):
    """An atlas frame with a crop (its own size, no offset) and a patched frame that is itself a cropped layer blending onto a canvas
    saved in slot 1 while the atlas is in slot 0."""
    pf = PU.patched(parts["atlas"], [PU.Ref(0, 10, 5, 20, 15, [PU.Place(0, 0, [R, R]), PU.Place(10, 5, [A, A])])], 1)
    f = LU.layered(parts["canvas"], [LU.Layer(parts["atlas"], frame_type=2, x0=0, y0=0), LU.Layer(parts["frame"], crop=False, save_ref=1),
                                     LU.Layer(pf, x0=-5, y0=70, flags=2, blending=[LU.Blending(2, 0, False, 1), LU.Blending(2, 0, False, 1)])])
    st, _, msg = api.parse_check(f)
    assert st == "Ok", msg
