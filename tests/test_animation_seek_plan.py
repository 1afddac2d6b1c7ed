"""Seeking and thumbnails of animations on the host: the entry points, and the chunks that seek / next / next_reduced plan, through
jxlhip_selftest_animation_seek_plan against the model in animation_seek_util.  Nothing here touches a GPU."""
import numpy as np
import pytest

import animation_seek_util as SU
import animation_util as AU
from animation_seek_util import NEXT, NEXT_REDUCED, SEEK
from test_animation_plan import H, W, long_frames, mixed_frames
from test_gpu_layers import F, build


def _px(rng, w, h, nch=4, bits=8):
    return rng.integers(0, 1 << bits, (h, w, nch), dtype=np.uint8 if bits <= 8 else np.uint16)


def all_replace_frames(n=5):
    rng = np.random.default_rng(3)
    return [F(_px(rng, 9, 7), crop=False, duration=1) for _ in range(n)]


def first_to_last_frames(n=6):
    """Frame 0 is saved to slot 1 and only the last frame reads it: no image but the first can be entered."""
    rng = np.random.default_rng(4)
    frames = [F(_px(rng, 9, 7), crop=False, duration=1) for _ in range(n)]
    frames[0] = F(_px(rng, 9, 7), crop=False, duration=1, save=1)
    frames[-1] = F(_px(rng, 4, 4), x0=3, y0=2, mode=2, source=1, duration=1)
    return frames


@pytest.fixture(scope="module")
def keyed(oracle):
    frames = SU.keyed_frames()
    return frames, build(oracle, SU.KW, SU.KH, frames, animation=True)


# ---------------------------------------------------------------- entry points
def test_entry_points_against_the_model(oracle, keyed):
    cases = [(mixed_frames(), W, H, [0]), (long_frames(), 9, 7, [0, 1, 2, 69]), (all_replace_frames(), 9, 7, [0, 1, 2, 3, 4]),
             (first_to_last_frames(), 9, 7, [0]), (keyed[0], SU.KW, SU.KH, SU.KEYED_ENTRY_POINTS)]
    for frames, w, h, by_hand in cases:
        data = keyed[1] if frames is keyed[0] else build(oracle, w, h, frames, animation=True)
        got = SU.seek_plan(data, []).entry_points
        model = [j for j in range(max(AU.shows(frames)) + 1)
                 if j == 0 or AU.live_behind(frames, w, h, SU.first_frame(frames, j) - 1) == 0]
        assert got == model == by_hand


def test_a_single_frame_file_has_one_entry_point(oracle):
    rng = np.random.default_rng(5)
    p = SU.seek_plan(oracle.encode(_px(rng, 20, 10), lossless=True), [(SEEK, 1), (SEEK, 0), (NEXT_REDUCED, 0, 3)])
    assert p.entry_points == [0]
    assert p.results == [(1, 0, 1), (1, 0, 0), (1, 1, 1)] and [c["stores"] for c in p.chunks] == [[0]]


# ---------------------------------------------------------------- plans
def _check(keyed, ops, **kw):
    frames, data = keyed
    p = SU.seek_plan(data, ops, **kw)
    results, chunks = SU.model_run(frames, SU.KW, SU.KH, ops, kw.get("chunk_frames", 0))
    assert p.results == results and SU.brief(p.chunks) == chunks
    return p


def test_a_seek_backwards_enters_at_the_latest_entry_point(keyed):
    frames, _ = keyed
    p = _check(keyed, [(NEXT, 10), (SEEK, 5), (NEXT, 1)])
    assert p.results[1] == (1, SU.first_frame(frames, 4), 5)
    assert [(c["first"], c["stores"]) for c in p.chunks[1:]] == [(SU.first_frame(frames, 4), [5])]
    # an entry point itself, and image 0
    p = _check(keyed, [(NEXT, 0), (SEEK, 8), (NEXT, 1), (SEEK, 3), (NEXT, 2)])
    assert p.results[1] == (1, SU.first_frame(frames, 8), 8) and p.results[3] == (1, 0, 3)
    assert [c["stores"] for c in p.chunks[1:]] == [[8], [3, 4]]


def test_a_forward_seek_goes_on_from_the_position_or_jumps_to_an_entry_point(keyed):
    frames, _ = keyed
    p = _check(keyed, [(NEXT, 1), (SEEK, 3), (NEXT, 1)])            # no entry point in (1, 3]: from where it stands
    assert p.results[1] == (1, SU.first_frame(frames, 1), 3) and p.chunks[1]["first"] == SU.first_frame(frames, 1)
    p = _check(keyed, [(NEXT, 1), (SEEK, 9), (NEXT, 1)])            # entry point 8 in between: from there
    assert p.results[1] == (1, SU.first_frame(frames, 8), 9) and p.chunks[1]["first"] == SU.first_frame(frames, 8) and p.chunks[1]["live_in"] == 0
    p = _check(keyed, [(SEEK, 7), (SEEK, 6), (SEEK, 7), (SEEK, 11)])   # lazy seeks: the decode stands at image 4, then at image 8
    assert [r[1] for r in p.results] == [SU.first_frame(frames, j) for j in (4, 4, 4, 8)] and p.chunks == []


def test_seek_to_the_position_and_to_the_end(keyed):
    frames, _ = keyed
    p = _check(keyed, [(NEXT, 2), (SEEK, 2), (NEXT, 1), (SEEK, 12), (NEXT, 3), (NEXT_REDUCED, 3, 2)])
    assert p.results[1] == p.results[0] == (1, SU.first_frame(frames, 2), 2)
    assert p.results[3][2] == 12 and p.results[4][2] == 12 and p.results[5][2] == 12
    assert [c["op"] for c in p.chunks] == [0, 2]                      # neither the seeks nor the calls at the end plan a chunk


def test_seek_and_next_over_a_gap_is_one_chunk_that_stores_one_image(keyed):
    for j in range(12):
        p = _check(keyed, [(SEEK, j), (NEXT, 1)])
        e = max(x for x in SU.KEYED_ENTRY_POINTS if x <= j)
        assert len(p.chunks) == 1 and p.chunks[0]["stores"] == [j] and p.chunks[0]["first_shown"] == e and p.chunks[0]["shown"] == j - e + 1
        assert p.chunks[0]["live_in"] == 0


def test_cuts_inside_a_seek_carry_the_live_slots(keyed):
    frames, data = keyed
    p = _check(keyed, [(SEEK, 7), (NEXT, 1), (SEEK, 10), (NEXT, 2)], chunk_frames=1)
    first = SU.first_frame(frames, 4)
    mine = [c for c in p.chunks if c["op"] == 1]
    assert [c["first"] for c in mine] == list(range(first, SU.first_frame(frames, 8))) and all(c["count"] == 1 for c in mine)
    assert [c["stores"] for c in mine] == [[]] * (len(mine) - 1) + [[7]]
    assert mine[0]["live_in"] == 0 and [c["live_out"] for c in mine[:-1]] == [2] * (len(mine) - 1) and mine[-1]["live_out"] == 0
    for a, b in zip(mine, mine[1:]):
        assert b["live_in"] == a["live_out"] == AU.live_behind(frames, SU.KW, SU.KH, a["first"])
    assert any(c["live_out"] == 4 for c in p.chunks if c["op"] == 3)   # image 10 goes through slot 2
    # a small scratch budget: the cuts fall where the frames' scratch says
    scratch = [f["scratch"] for f in AU.plan(data).frames]
    budget = scratch[first] + scratch[first + 1]
    ops = [(SEEK, 7), (NEXT_REDUCED, 2, 3)]
    got = SU.seek_plan(data, ops, scratch_budget=budget)
    results, chunks = SU.model_run(frames, SU.KW, SU.KH, ops, 0, scratch, budget)
    assert got.results == results and SU.brief(got.chunks) == chunks and len(chunks) > 2
    assert [s for c in got.chunks for s in c["stores"]] == [7, 10]


@pytest.mark.parametrize("chunk_frames", [0, 1, 3])
def test_next_reduced_stores_every_step_th_image(keyed, chunk_frames):
    frames, _ = keyed
    p = _check(keyed, [(SEEK, 1), (NEXT_REDUCED, 3, 4)], chunk_frames=chunk_frames)
    assert [s for c in p.chunks for s in c["stores"]] == [1, 5, 9] and p.results[1] == (1, SU.first_frame(frames, 10), 12)
    p = _check(keyed, [(NEXT_REDUCED, 2, 5), (NEXT, 1)], chunk_frames=chunk_frames)
    assert [s for c in p.chunks for s in c["stores"]] == [0, 5, 10] and p.results[0] == (1, SU.first_frame(frames, 6), 10)
    p = _check(keyed, [(NEXT_REDUCED, 0, 5)], chunk_frames=chunk_frames)
    assert [s for c in p.chunks for s in c["stores"]] == [0, 5, 10] and p.results[0][2] == 12
    p = _check(keyed, [(NEXT_REDUCED, 0, 1)], chunk_frames=chunk_frames)
    assert [s for c in p.chunks for s in c["stores"]] == list(range(12))
    if chunk_frames == 0:
        assert len(p.chunks) == 1


def test_the_long_file_against_the_model(oracle):
    frames = long_frames()
    data = build(oracle, 9, 7, frames, animation=True)
    ops = [(SEEK, 68), (NEXT, 1), (SEEK, 69), (SEEK, 30), (NEXT_REDUCED, 4, 5), (SEEK, 69), (NEXT, 1)]
    p = SU.seek_plan(data, ops)
    results, chunks = SU.model_run(frames, 9, 7, ops)
    assert p.results == results and SU.brief(p.chunks) == chunks
    # image 68 needs slot 3 from frame 2: two chunks (64 + 3 frames), the slot across the cut, one image stored
    assert [(c["first"], c["count"], c["live_in"], c["live_out"], c["stores"]) for c in p.chunks[:2]] == [(2, 64, 0, 8, []), (66, 3, 8, 0, [68])]
    assert p.chunks[-1]["first"] == 69 and p.chunks[-1]["stores"] == [69]


def test_existing_plans_are_unchanged(keyed):
    """NextChunk's old callers: the chunks of plain next calls are those of jxlhip_selftest_animation_plan."""
    frames, data = keyed
    for chunk_frames, counts in ((0, (0,)), (2, (3, 0)), (1, (1, 1, 0))):
        old = AU.plan(data, chunk_frames, counts).chunks
        new = SU.seek_plan(data, [(NEXT, c) for c in counts], chunk_frames=chunk_frames).chunks
        assert [[c[k] for k in ("first", "count", "first_shown", "shown", "live_in", "live_out")] for c in new] == \
               [[c[k] for k in ("first", "count", "first_shown", "shown", "live_in", "live_out")] for c in old]
        assert all(c["stores"] == list(range(c["first_shown"], c["first_shown"] + c["shown"])) for c in new if c["shown"])


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_position_alone(keyed):
    frames, _ = keyed
    p = _check(keyed, [(NEXT, 3), (SEEK, -1), (SEEK, 13), (NEXT_REDUCED, 2, 0), (NEXT_REDUCED, 2, -4), (NEXT, 1)])
    at = (SU.first_frame(frames, 3), 3)
    assert p.results[0] == (1,) + at
    assert p.results[1:5] == [(0,) + at] * 4
    assert p.chunks[-1]["stores"] == [3] and [c["op"] for c in p.chunks] == [0, 5]
