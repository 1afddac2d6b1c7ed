"""The paths of one step of the batched HF token loop (hf_decode_kernel, HfBatchedLoop / HfTakeToken / HfFillColumns), each reached on
purpose: column fills of 1, 2, 4, 8, 16 and 32 cells by square and rectangular varblocks, a block in column 0 of its group and one whose left
neighbour is the block decoded just before it (its prediction is patched from registers), channels without a non-zero, blocks whose
non-zeros run to the last position, and a section whose data ends early.

Frames of 2 to 6 groups written by the oracle and by the product encoder are decoded with 2, 4, 8 and 64 lanes between sections (64:
the one-section loop; the others: the batched loop with 32, 16 and 8 sections to a wavefront), byte for byte against each other and
against the oracle within test_gpu_hf_batched's bar.  What a frame is there for is asserted from the oracle's dump of that very stream
(strategy plane, quantised coefficients), so a picture that stops reaching its path fails here and not silently.

A coefficient outside int16 (kErrRange) is something neither writer produces: the oracle's writer and the product encoder both clamp
quantised HF values to +-32767 before they form tokens ("Quantiser").  That stream is a stored one,
tests/golden/hf_wide_coefficient_512x256_f32.jxl: what the oracle's writer makes of wide_source() below at distance 1 with its clamp
(kMaxQuantHf in oracle/jxo_enc.cc) raised to 2^24 in a build of its own.  The oracle's reader has no such bound, so its dump of the
stored stream states what the stream holds."""
import numpy as np
import pytest

from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth
from gpu_helpers import gpu_decode
from test_gpu_hf_batched import check_pixels, noise
import varblock_util as V

pytestmark = pytest.mark.gpu

STRIDES = (64, 8, 4, 2)
S = V.S

# group (0, 0) of a 768 x 512 frame: every block width up to 8 cells, squares and both kinds of rectangle; group (1, 0) starts with a
# 64 x 64 block in its column 0; the blocks of 16 and 32 cells (128 and 256 samples) lie in the other groups; the rest is DCT8
LAYOUT = [(S["DCT64X64"], 0, 0), (S["DCT32X64"], 8, 0), (S["DCT32X32"], 16, 0), (S["DCT8X32"], 20, 0), (S["DCT16X32"], 24, 0),
          (S["DCT16X16"], 28, 0), (S["DCT8X16"], 30, 0), (S["DCT32X16"], 16, 4), (S["DCT16X8"], 18, 4), (S["DCT32X8"], 19, 4),
          (S["DCT64X32"], 8, 4), (S["DCT64X64"], 32, 0), (S["DCT16X16"], 0, 32), (S["DCT8X16"], 62, 40),
          (S["DCT256X256"], 64, 0), (S["DCT128X128"], 32, 32), (S["DCT64X128"], 0, 40), (S["DCT128X256"], 64, 32)]


def half_flat(w, h, seed):
    """The left half one colour (blocks and channels without a non-zero), the right half a picture."""
    img = synth(w, h, seed).copy()
    img[:, : w // 2, :3] = (90, 120, 60)
    img[..., 3] = 255
    return img


def build_streams(oracle):
    return {
        "layout": oracle.encode(synth(768, 512, 61), distance=0.5, varblocks=LAYOUT),                 # 6 groups
        "dense": oracle.encode(noise(512, 256, 7), distance=0.1, strategy_mode=1),                    # 2 groups, DCT8 only
        "half-flat": oracle.encode(half_flat(520, 500, 62), distance=1.0),                            # 6 groups, the writer's own blocks
        "product": api.save_image(np.ascontiguousarray(half_flat(640, 512, 63)[..., [2, 1, 0, 3]]), distance=1.0, effort=7),   # 6 groups
    }


@pytest.fixture(scope="module")
def corpus(oracle):
    """name -> (stream, the oracle's dump of it); built once, read only."""
    return {name: (data, oracle.decode(data, want_dump=True)) for name, data in build_streams(oracle).items()}


def origins(od):
    plane = od.planes["strategy"].reshape(od.h8, od.w8)
    return plane, V.blocks_of(plane)


def per_cell(od, c):
    return od.planes["qcoef"][c].reshape(od.h8, 8, od.w8, 8).transpose(0, 2, 1, 3).reshape(od.h8, od.w8, 64)


def dct8_cells(od):
    plane, _ = origins(od)
    return plane == (0x80 | S["DCT8"])


# ---------------------------------------------------------------- what each frame is there for
def test_layout_reaches_every_fill_width_and_both_neighbour_cases(corpus):
    _, od = corpus["layout"]
    assert (od.w8, od.h8) == (96, 64)
    plane, blocks = origins(od)
    assert np.array_equal(plane, V.tiling(LAYOUT, od.w8, od.h8))
    shapes = {(V.COVERED_X[s], V.COVERED_Y[s]) for s, _, _ in blocks}
    for width in (1, 2, 4, 8, 16, 32):
        assert any(cx == width and cy == cx for cx, cy in shapes), ("square", width)
        assert any(cx == width and cy != cx for cx, cy in shapes), ("rectangle", width)
    # column 0 of a group, by a block wider than one cell, in the first and in a later group
    assert any(bx == 0 and V.COVERED_X[s] == 8 for s, bx, by in blocks) and any(bx == 32 and V.COVERED_X[s] == 8 for s, bx, by in blocks)
    # the left neighbour is the block decoded just before: consecutive origins of one row, the second not in column 0 of a group;
    # with a wide block on the left (all of its columns were filled after the read ahead) and with a DCT8 on the left
    pairs = [(a, b) for a, b in zip(blocks, blocks[1:]) if a[2] == b[2] and a[1] + V.COVERED_X[a[0]] == b[1] and b[1] % 32]
    assert any(V.COVERED_X[a[0]] == 8 for a, b in pairs) and any(V.COVERED_X[a[0]] == 1 for a, b in pairs)
    # ... and blocks whose left neighbour hangs down from an earlier row (read ahead from the columns, not patched)
    assert any(by > 0 and bx % 32 and plane[by, bx - 1] & 0x80 == 0 for s, bx, by in blocks)
    # the wide blocks carry non-zeros (their fills are not all zero)
    for s, bx, by in blocks:
        if V.COVERED_X[s] >= 4:
            cx, cy = V.COVERED_X[s], V.COVERED_Y[s]
            assert any(np.count_nonzero(per_cell(od, c)[by:by + cy, bx:bx + cx]) > 1 for c in range(3)), (s, bx, by)


def test_dense_frame_fills_blocks_to_the_last_position(corpus):
    _, od = corpus["dense"]
    assert (od.w8, od.h8) == (64, 32) and dct8_cells(od).all()
    for c in range(3):
        q = per_cell(od, c)
        assert (q[..., 63] != 0).any(), c                          # the last scan position of a DCT8 (7, 7) holds a non-zero
    assert (np.count_nonzero(per_cell(od, 1)[..., 1:], axis=2) == 63).any()   # a block of Y with every HF position non-zero


@pytest.mark.parametrize("name", ["half-flat", "product"])
def test_flat_halves_leave_channels_without_a_non_zero(corpus, name):
    _, od = corpus[name]
    assert (od.w8 + 31) // 32 * ((od.h8 + 31) // 32) == 6
    cells = dct8_cells(od)
    assert cells.any()
    empty = [np.count_nonzero(per_cell(od, c)[..., 1:], axis=2) == 0 for c in range(3)]
    assert all((e & cells).any() for e in empty)                                # every channel has blocks without a non-zero ...
    assert (cells & empty[0] & empty[2] & ~empty[1]).any()                      # ... and some blocks have them in chroma only
    assert any(V.COVERED_X[s] > 1 for s, _, _ in origins(od)[1])                # the writer's own choice holds wide blocks too


# ---------------------------------------------------------------- the decodes
@pytest.fixture(scope="module")
def decodes(gpu_decoder, corpus):
    """name -> {lane stride: pixels}; one batch per stride."""
    names = sorted(corpus)
    out = {n: {} for n in names}
    for stride in STRIDES:
        for n, px in zip(names, gpu_decode(gpu_decoder, [corpus[n][0] for n in names], lane_stride=stride)):
            out[n][stride] = px
    gpu_decoder.set_option("lane_stride", 0)
    return out


@pytest.mark.parametrize("name", ["layout", "dense", "half-flat", "product"])
def test_lane_mappings_agree_and_match_the_oracle(corpus, decodes, name):
    ref = corpus[name][1].pixels
    base = decodes[name][64]
    check_pixels(base, ref)
    for stride in STRIDES[1:]:
        assert np.array_equal(decodes[name][stride], base), stride


def test_frames_alone_decode_as_in_the_batch(gpu_decoder, corpus, decodes):
    """One frame per launch: fewer sections than a wavefront has lanes (6 and 2), at the strides of the batched loop."""
    for name in ("layout", "dense"):
        for stride in (2, 8):
            assert np.array_equal(gpu_decode(gpu_decoder, [corpus[name][0]], lane_stride=stride)[0], decodes[name][64]), (name, stride)
    gpu_decoder.set_option("lane_stride", 0)


# ---------------------------------------------------------------- a section cut short
def test_truncated_last_section_is_an_error_at_every_stride(gpu_decoder, oracle, corpus, decodes):
    """The data of the last pass-group section ends 2000 bytes early (zeros from there on; a file cut short never reaches the kernel,
    the host refuses a table of contents that exceeds the file): every mapping ends with an error status and writes nothing to the
    caller's buffer; the frame beside it decodes as before, and so does the next batch."""
    import torch
    data = corpus["dense"][0]
    cut = data[: len(data) - 2000] + bytes(2000)
    assert api.parse_check(cut)[0] == "Ok"
    with pytest.raises(oracle.OracleError):
        oracle.decode(cut)
    good = corpus["layout"][0]
    infos = [api.peek(f) for f in (good, cut)]
    for stride in STRIDES:
        gpu_decoder.set_option("lane_stride", stride)
        outs = [torch.full((i.width * i.height * i.num_channels,), 0xA5, dtype=torch.uint8, device="cuda") for i in infos]
        torch.cuda.synchronize()
        st = gpu_decoder.decode_batch([good, cut], [o.data_ptr() for o in outs], None, raise_on_error=False)
        assert st[0] == 0 and st[1] != 0, (stride, st)
        assert (outs[1].cpu().numpy() == 0xA5).all(), stride
        assert np.array_equal(outs[0].cpu().numpy().reshape(decodes["layout"][64].shape), decodes["layout"][64]), stride
    assert np.array_equal(gpu_decode(gpu_decoder, [data], lane_stride=4)[0], decodes["dense"][64])
    gpu_decoder.set_option("lane_stride", 0)


# ---------------------------------------------------------------- a coefficient outside int16
WIDE_FILE = "hf_wide_coefficient_512x256_f32.jxl"


def wide_source():
    """The float32 picture behind WIDE_FILE: a picture in the first group; in the second a flat field and a 64 x 64 square of steps
    between 0 and 4000 (extremes_util's hdr-step, four times as high)."""
    px = synth(512, 256, 64)[..., :3].astype(np.float32) / 255.0
    px[:, 256:] = 0.25
    px[96:160, 352:416] = 0.0
    px[96:160, 352:416][:, np.arange(64) % 8 >= 4] = 4000.0
    return np.ascontiguousarray(px)


def test_coefficient_outside_int16_is_a_range_error_at_every_stride(gpu_decoder, oracle, corpus, decodes):
    """Every mapping refuses the frame with the range flag alone, names the section of the second group, leaves the caller's buffer as
    it was and decodes the frame beside it as before; so does LoadImage; the next batch decodes as before."""
    import os
    import re
    import torch
    wide = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", WIDE_FILE), "rb").read()
    # what the stored stream holds, from the oracle's dump: Y coefficients beyond int16 in the second group only, the rest far inside
    od = oracle.decode(wide, want_dump=True)
    assert (od.w8, od.h8) == (64, 32) and od.pixels.dtype == np.float32
    q = [np.abs(od.planes["qcoef"][c]).reshape(od.h8 * 8, od.w8 * 8) for c in range(3)]
    assert int(q[1].max()) > 32768 and int((q[1][:, 256:] > 32768).sum()) >= 8 and int(q[1][:, :256].max()) < 32767
    assert int(q[0].max()) < 32767 and int(q[2].max()) < 32767
    # ... and the clamped writer makes another stream of the same picture (the stored one is not what today's oracle writes)
    clamped = oracle.decode(oracle.encode(wide_source(), distance=1.0, float_samples=32), want_dump=True)
    assert max(int(np.abs(clamped.planes["qcoef"][c]).max()) for c in range(3)) == 32767
    assert api.parse_check(wide)[0] == "Ok"
    with pytest.raises(api.FormatError) as e:
        api.load_image(wide)
    assert e.value.status == "DecodeError" and "value-out-of-range" in str(e.value), str(e.value)
    good = corpus["layout"][0]
    infos = [api.peek(f) for f in (good, wide)]
    assert infos[1].bytes_per_sample == 4
    for stride in STRIDES:
        gpu_decoder.set_option("lane_stride", stride)
        outs = [torch.full((i.width * i.height * i.num_channels * i.bytes_per_sample,), 0xA5, dtype=torch.uint8, device="cuda") for i in infos]
        torch.cuda.synchronize()
        st = gpu_decoder.decode_batch([good, wide], [o.data_ptr() for o in outs], None, raise_on_error=False)
        assert st == [0, api.DECODER_STATUS.index("DecodeError")], (stride, st)
        msg = gpu_decoder.last_error
        assert "value-out-of-range" in msg and "corrupt-bitstream" not in msg, (stride, msg)
        m = re.search(r"hf (\d+)", msg)
        assert m and int(m.group(1)) == 2, (stride, msg)      # the second group's section (sections are named from 1)
        assert (outs[1].cpu().numpy() == 0xA5).all(), stride
        assert np.array_equal(outs[0].cpu().numpy().reshape(decodes["layout"][64].shape), decodes["layout"][64]), stride
    assert np.array_equal(gpu_decode(gpu_decoder, [corpus["dense"][0]], lane_stride=4)[0], decodes["dense"][64])
    gpu_decoder.set_option("lane_stride", 0)
