"""Animations on the host: the frame walk (ParseAnimation), the header fields, the refusals and the decode plan - chunks of frames and
the reference slots alive between them - against the model in animation_util.  Nothing here touches a GPU."""
import numpy as np
import pytest

import animation_util as AU
import layer_util as LU
from pdn_jpegxl_amd import api
from test_gpu_layers import F, build

W, H = 67, 45


def _px(rng, w, h, nch=4, bits=8):
    return rng.integers(0, 1 << bits, (h, w, nch), dtype=np.uint8 if bits <= 8 else np.uint16)


def mixed_frames(bits=8, seed=5):
    """Six frames, three displayed images (durations 0, 3, 0, 0, 5, 1): every blend mode, clamp, crops with negative offsets and past
    the canvas, zero-duration layers between displayed frames, a frame with a duration and save slot 2 (saved) and one with a duration
    and save slot 0 (not saved), every slot in use."""
    rng = np.random.default_rng(seed)
    return [F(_px(rng, W, H, 4, bits), crop=False, save=0, name=b"base"),
            F(_px(rng, 40, 30, 4, bits), x0=-7, y0=20, mode=2, source=0, duration=3, save=2, name=b"first"),
            F(_px(rng, 20, 50, 4, bits), x0=55, y0=-3, mode=1, clamp=True, source=2, save=1),
            F(_px(rng, 30, 20, 4, bits), x0=10, y0=10, mode=3, source=1, asource=0, save=3),
            F(_px(rng, 25, 25, 4, bits), x0=-5, y0=-5, mode=4, clamp=True, source=3, duration=5, save=0, name=b"second"),
            F(_px(rng, 33, 21, 4, bits), x0=30, y0=20, mode=2, source=2, duration=1, name=b"third")]


def long_frames(n=70, seed=6):
    """n frames of 9 x 7, one per displayed image, except: frame 2 is saved to slot 3 and frame n - 2 blends onto that slot."""
    rng = np.random.default_rng(seed)
    frames = [F(_px(rng, 9, 7), crop=False, duration=1) for _ in range(n)]
    frames[2] = F(_px(rng, 9, 7), crop=False, duration=1, save=3)
    frames[n - 2] = F(_px(rng, 5, 4), x0=2, y0=1, mode=2, source=3, duration=1)
    return frames


@pytest.fixture(scope="module")
def mixed(oracle):
    frames = mixed_frames()
    return frames, build(oracle, W, H, frames, animation=True)


def test_frame_table(mixed):
    frames, data = mixed
    p = AU.plan(data)
    assert (p.width, p.height, p.have_animation, p.raw) == (W, H, 1, 0)
    assert p.num_displayed == 3 and len(p.frames) == 6
    assert [f["show"] for f in p.frames] == AU.shows(frames) == [-1, 0, -1, -1, 1, 2]
    assert [f["duration"] for f in p.frames] == [0, 3, 0, 0, 5, 1]
    assert [f["save"] for f in p.frames] == AU.saves(frames) == [0, 2, 1, 3, -1, -1]
    assert [f["name"] for f in p.frames] == [fr.name for fr in frames]
    for f, fr in zip(p.frames, frames):
        assert f["reads"] == sum(1 << s for s in AU.reads(fr, W, H))
        assert (f["source"], f["asource"], f["mode"], f["amode"]) == (fr.source, fr.asource, fr.mode, fr.amode)
    assert [f["live_after"] for f in p.frames] == [AU.live_behind(frames, W, H, e) for e in range(6)]
    assert all(f["scratch"] > 0 for f in p.frames)


@pytest.mark.parametrize("counts", [(0,), (1, 1, 1), (2, 5), (1, 0)])
@pytest.mark.parametrize("chunk_frames", [1, 2, 3, 0])
def test_chunks_and_live_slots(mixed, chunk_frames, counts):
    frames, data = mixed
    p = AU.plan(data, chunk_frames, counts)
    want = AU.model_chunks(frames, W, H, chunk_frames, counts)
    got = [{k: c[k] for k in want[0]} for c in p.chunks]
    assert got == want
    # the chunks tile the file, and each takes up where the one before left off
    assert sum(c["count"] for c in p.chunks) == 6 and sum(c["shown"] for c in p.chunks) == 3
    for a, b in zip(p.chunks, p.chunks[1:]):
        assert b["first"] == a["first"] + a["count"] and b["live_in"] == a["live_out"]
    assert p.chunks[0]["live_in"] == 0 and p.chunks[-1]["live_out"] == 0


def test_cuts_by_the_scratch_budget(mixed):
    """The budget is a parameter of the plan: a chunk stops in front of the frame that would take its scratch past it, and a frame
    larger than the budget is a chunk of its own.  The frames' scratch (frame 0 is the canvas-sized one) comes from the plan."""
    frames, data = mixed
    scratch = [f["scratch"] for f in AU.plan(data).frames]
    assert scratch[0] > max(scratch[1:]) and all(s > 0 for s in scratch)
    keys = ("call", "first", "count", "shown", "live_in", "live_out")
    budgets = [scratch[0] - 1, scratch[0], scratch[1] + scratch[2], scratch[1] + scratch[2] - 1, sum(scratch) - 1, sum(scratch), 1]
    seen = set()
    for budget in budgets:
        for chunk_frames, counts in ((0, (0,)), (3, (0,)), (0, (1, 2))):
            p = AU.plan(data, chunk_frames, counts, scratch_budget=budget)
            got = [{k: c[k] for k in keys} for c in p.chunks]
            assert got == AU.model_chunks(frames, W, H, chunk_frames, counts, scratch, budget), (budget, chunk_frames, counts)
            for c in p.chunks:   # within the budget, or one frame
                assert c["count"] == 1 or sum(scratch[c["first"]:c["first"] + c["count"]]) <= budget
            seen.add(tuple(c["count"] for c in p.chunks))
    assert [c["count"] for c in AU.plan(data, scratch_budget=1).chunks] == [1] * 6            # every frame over the budget
    assert [c["count"] for c in AU.plan(data, scratch_budget=sum(scratch)).chunks] == [6]     # exactly the budget: no cut
    assert [c["count"] for c in AU.plan(data, scratch_budget=sum(scratch) - 1).chunks] == [5, 1]
    assert len(seen) > 4


def test_live_masks_of_the_mixed_file_by_hand(mixed):
    """Worked out on paper: slot 0 (frame 0) is read by frames 1 and 3; slot 2 (frame 1) by frames 2 and 5; slot 1 (frame 2) by
    frame 3; slot 3 (frame 3) by frame 4."""
    _, data = mixed
    p = AU.plan(data, 1)
    assert [c["live_out"] for c in p.chunks] == [0b0001, 0b0101, 0b0111, 0b1100, 0b0100, 0]


def test_seventy_displayed_frames_are_not_refused(oracle):
    frames = long_frames()
    data = build(oracle, 9, 7, frames, animation=True)
    p = AU.plan(data)
    assert p.num_displayed == 70 and len(p.frames) == 70
    assert [(c["first"], c["count"], c["shown"]) for c in p.chunks] == [(0, 64, 64), (64, 6, 6)]
    # slot 3 lives from frame 2 to frame 68, across the cut
    assert p.chunks[0]["live_out"] == 8 and p.chunks[1]["live_in"] == 8
    assert [c["live_out"] for c in AU.plan(data, 3).chunks] == [AU.live_behind(frames, 9, 7, e) for e in range(2, 70, 3)] + [0]
    got = AU.plan(data, 0, (1,) * 70)
    assert [{k: c[k] for k in ("call", "first", "count", "shown", "live_in", "live_out")} for c in got.chunks] == AU.model_chunks(frames, 9, 7, 0, (1,) * 70)


def test_still_of_sixty_six_frames_plans_as_two_chunks(oracle):
    """Sixty-five layers and the displayed frame: past what a layered still may hold (all its frames are resident at once)."""
    rng = np.random.default_rng(8)
    frames = [F(_px(rng, 9, 7), crop=False)] + [F(_px(rng, 3, 3), x0=k % 7, y0=k % 5, mode=1) for k in range(65)]
    data = build(oracle, 9, 7, frames)
    assert "more than 64 frames" in api.parse_check(data)[2]
    p = AU.plan(data)
    assert p.have_animation == 0 and p.num_displayed == 1 and len(p.frames) == 66
    assert [f["show"] for f in p.frames] == [-1] * 65 + [0]
    assert [(c["first"], c["count"], c["shown"], c["live_in"], c["live_out"]) for c in p.chunks] == [(0, 64, 0, 0, 1), (64, 2, 1, 1, 0)]


def test_single_frame_and_layered_still_have_one_displayed_image(oracle):
    rng = np.random.default_rng(9)
    one = AU.plan(oracle.encode(_px(rng, 20, 10), lossless=True))
    assert (one.num_displayed, len(one.frames), one.have_animation, one.raw, one.single) == (1, 1, 0, 1, 1)
    assert (one.tps_numerator, one.tps_denominator, one.num_loops, one.have_timecodes) == (0, 0, 0, 0)
    lossy = AU.plan(oracle.encode(_px(rng, 40, 30), distance=1.0))
    assert (lossy.num_displayed, len(lossy.frames)) == (1, 1)
    still = AU.plan(build(oracle, 20, 10, [F(_px(rng, 20, 10), crop=False), F(_px(rng, 5, 5), x0=3, y0=3, mode=2)]))
    assert (still.num_displayed, len(still.frames), still.raw, still.single) == (1, 2, 0, 0)
    # a lone frame that blends onto the empty canvas is a layered image, to ParseFile as well
    lone = AU.plan(build(oracle, 20, 10, [F(_px(rng, 20, 10), crop=False, mode=1)]))
    assert (lone.num_displayed, len(lone.frames), lone.single, lone.raw) == (1, 1, 0, 0)


def test_a_single_cmyk_frame_is_accepted_as_load_image_accepts_it(oracle):
    """A layered image cannot be CMYK, a single frame can: a file that is one single-frame image goes the single-frame way."""
    import icc_util
    rng = np.random.default_rng(14)
    data = oracle.encode(_px(rng, 20, 10, 5), lossless=True, icc=icc_util.cmyk_profile(), cmyk=True)
    assert api.parse_check(data)[0] == "Ok"
    p = AU.plan(data)
    assert (p.num_displayed, len(p.frames), p.single) == (1, 1, 1)


def test_the_oracles_animation(oracle):
    """The oracle's writer: 100 / 1 ticks per second, endless, no timecodes, every frame shown for 10 ticks."""
    rng = np.random.default_rng(10)
    p = AU.plan(oracle.encode(_px(rng, 9, 7), animation_frames=3, lossless=True))
    assert (p.have_animation, p.tps_numerator, p.tps_denominator, p.num_loops, p.have_timecodes) == (1, 100, 1, 0, 0)
    assert p.num_displayed == 3 and [f["duration"] for f in p.frames] == [10, 10, 10] and p.raw == 1
    assert [f["show"] for f in p.frames] == [0, 1, 2] and [f["save"] for f in p.frames] == [-1, -1, -1]


# every selector of the three U32 fields once: 100 | 1000 | 1 + u(10) | 1 + u(30); 1 | 1001 | 1 + u(8) | 1 + u(10); 0 | u(3) | u(16) | u(32)
@pytest.mark.parametrize("num,den,loops,timecodes", [(100, 1, 0, True), (1000, 1001, 5, False), (24, 25, 300, True), (70000, 600, 70000, False)])
def test_header_fields_come_back_as_written(oracle, num, den, loops, timecodes):
    rng = np.random.default_rng(num)
    kw = dict(lossless=True, container=False)
    canvas = AU.with_animation_header(oracle.encode(np.zeros((7, 9, 4), np.uint8), animation_frames=2, **kw), num, den, loops, timecodes)
    layers = [LU.Layer(oracle.encode(_px(rng, 9, 7), **kw), crop=False, duration=d, name=b"n%d" % d) for d in (4, 0, 300)]
    tcs = [0x01020304, 0, 0xFFFFFFFF] if timecodes else [0, 0, 0]
    data = AU.frames_with_timecodes(canvas, layers, tcs)
    p = AU.plan(data)
    assert (p.have_animation, p.tps_numerator, p.tps_denominator, p.num_loops, p.have_timecodes) == (1, num, den, loops, int(timecodes))
    assert [f["timecode"] for f in p.frames] == tcs and [f["duration"] for f in p.frames] == [4, 0, 300]
    assert [f["show"] for f in p.frames] == [0, -1, 1] and [f["name"] for f in p.frames] == [b"n4", b"n0", b"n300"]
    # the same file through the unchanged muxer when there are no timecodes to write
    if not timecodes:
        assert data == LU.layered(canvas, layers)


def refused_files(oracle):
    """An animation whose frame 1, behind the first displayed image, is something the decoder does not take: (name, file, message)."""
    rng = np.random.default_rng(12)
    kw = dict(lossless=True, container=False)
    canvas = oracle.encode(np.zeros((30, 40, 4), np.uint8), animation_frames=2, **kw)
    full = lambda **k: LU.Layer(oracle.encode(_px(rng, 40, 30), **kw), crop=False, **k)
    small = lambda **k: LU.Layer(oracle.encode(_px(rng, 10, 10), **kw), x0=1, y0=1, **k)
    bad = {"patches": (small(duration=1, flags=2), "animations with patches are not supported (animation, frame 1)"),
           "reference_only": (full(frame_type=2), "animations with patches are not supported (animation, frame 1)"),
           "upsampled": (small(duration=1, upsampling2=True), "upsampled frames are not supported yet (layered image, frame 1)"),
           "lf_frame": (small(duration=1, flags=32), "LF frames are not supported yet (layered image, frame 1)")}
    return [(name, LU.layered(canvas, [full(duration=2), layer, small(duration=1)]), msg) for name, (layer, msg) in bad.items()]


def test_refusals_behind_the_first_displayed_image(oracle):
    for name, data, msg in refused_files(oracle):
        with pytest.raises(api.FormatError) as e:
            AU.plan(data)
        assert msg in str(e.value), (name, str(e.value))
        # LoadImage's parse never reads that far: the file is a single-frame image to it
        assert api.parse_check(data)[0] == "Ok", name
        assert api.peek(data).width == 40


def test_lossy_frames_that_blend_are_refused_with_the_stills_words(oracle):
    rng = np.random.default_rng(13)
    lc = oracle.encode(_px(rng, 40, 30), distance=1.0, container=False, animation_frames=2)
    one = lambda w, h: oracle.encode(_px(rng, w, h), distance=1.0, container=False)
    data = LU.layered(lc, [LU.Layer(one(40, 30), crop=False, duration=1),
                           LU.Layer(one(10, 10), x0=2, y0=2, duration=1, blending=[LU.Blending(2, 0, False, 0), LU.Blending(2, 0, False, 0)])])
    with pytest.raises(api.FormatError) as e:
        AU.plan(data)
    assert "blend modes other than replace on lossy (XYB) frames are not supported (layered image, frame 1)" in str(e.value)
