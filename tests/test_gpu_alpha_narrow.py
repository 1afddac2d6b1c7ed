"""Alpha residuals as int16 between the two alpha phases (alpha_ans_kernel's lane path -> alpha_finish_gradient_kernel<true>).

Same frames and checks as test_gpu_alpha_pipeline: oracle.encode(synth(w, h, 41), distance=1.0), alpha compared with the source
exactly, colour through check_pixels.  Small batches take the one-section scalar path, which keeps int32 residuals, so every case asks
for the bench's launch shape: no_direct = 1, lane_stride = 2.

Three settings of alpha_narrow_limit - the default (32767), 0 (never narrow: the int32 path) and 100 (some groups of synth's alpha
carry larger residuals: they are given up in mid-stream and decoded again as int32 by the redo launch) - must give identical bytes,
and the counters must show that each path was really taken:

  default   narrow groups == eligible groups, redo groups == 0
  0         narrow groups == 0, redo groups == 0
  100       narrow + redo == eligible; both non-zero on 528x264 and on 1040x17 (per-group maximum |residual| of the group-local clamped
            gradient of synth(., ., 41)'s alpha: 64, 117, 64, 64, 130, 64 and 64, 91, 117, 94, 64)

Eligible: a group that alpha_ans_kernel decodes (frames of more than one group; a one-group frame has its alpha channel in LfGlobal,
decoded by the LF kernel as int32) and that alpha_finish_gradient_kernel takes (8-bit alpha, frame width a multiple of 4, group width a
multiple of 16; the oracle writes one gradient leaf).
"""
import numpy as np
import pytest

from pdn_jpegxl_amd.synth import synth, synth16
from gpu_helpers import gpu_decode
from test_gpu_parity import check_pixels

pytestmark = pytest.mark.gpu

SHAPES = [(16, 1), (16, 17), (32, 33), (256, 3), (272, 17), (16, 272), (1040, 17), (528, 264), (24, 40), (20, 9)]
MIXED = [(16, 17), (272, 17), (24, 40), (528, 264)]
LIMITS = [None, 0, 100]   # None: the decoder's default

_cache = {}


def frame(oracle, size):
    """(source, file, oracle's pixels) of one shape: encoded and decoded by the oracle once for the whole module."""
    if size not in _cache:
        img = synth(size[0], size[1], 41)
        data = oracle.encode(img, distance=1.0)
        _cache[size] = (img, data, oracle.decode(data).pixels)
    return _cache[size]


def eligible_groups(w, h):
    xg, yg = (w + 255) // 256, (h + 255) // 256
    if xg * yg == 1 or w % 4:
        return 0
    return sum(yg for gx in range(xg) if min(256, w - gx * 256) % 16 == 0)


def decode_with_limit(dec, files, limit):
    """Decodes one batch on the lane path; returns (outputs, narrow groups, redo groups)."""
    assert dec.set_option("no_direct", 1)
    assert dec.set_option("alpha_narrow_limit", 32767 if limit is None else limit)
    try:
        outs = gpu_decode(dec, files, lane_stride=2)
        return outs, dec.set_option("query_alpha_narrow_groups", 0), dec.set_option("query_alpha_redo_groups", 0)
    finally:
        dec.set_option("no_direct", 0)
        dec.set_option("alpha_narrow_limit", 32767)
        dec.set_option("lane_stride", 0)


def run_sizes(dec, oracle, sizes):
    frames = [frame(oracle, s) for s in sizes]
    files = [f[1] for f in frames]
    eligible = sum(eligible_groups(*s) for s in sizes)
    first = None
    counts = {}
    for limit in LIMITS:
        outs, narrow, redo = decode_with_limit(dec, files, limit)
        print("sizes %s limit %s: eligible %d narrow %d redo %d" % (sizes, limit, eligible, narrow, redo))
        counts[limit] = (narrow, redo)
        if first is None:
            first = outs
            for (img, _, ref), out in zip(frames, outs):
                assert out.shape == img.shape
                assert (out[..., 3] == img[..., 3]).all()
                check_pixels(out, ref)
        else:
            for a, b in zip(first, outs):
                assert a.tobytes() == b.tobytes(), limit
    assert counts[None] == (eligible, 0)
    assert counts[0] == (0, 0)
    assert counts[100][0] + counts[100][1] == eligible
    return counts


@pytest.mark.parametrize("size", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_shapes(gpu_decoder, oracle, size):
    counts = run_sizes(gpu_decoder, oracle, [size])
    if size in ((528, 264), (1040, 17)):
        assert counts[100][0] > 0 and counts[100][1] > 0, counts


def test_different_frames_in_one_launch(gpu_decoder, oracle):
    """Narrow groups, groups decoded again, groups that stay int32 and a one-group frame in one launch of each alpha kernel."""
    counts = run_sizes(gpu_decoder, oracle, MIXED)
    assert counts[100][0] > 0 and counts[100][1] > 0, counts


def test_16_bit_alpha_stays_int32(oracle):
    """A frame with 16-bit alpha is not one the gradient pipeline takes: no narrow group, and it decodes as it did (the bounds of
    test_gpu_formats.test_lossy_16_bit_matches_oracle, same frame)."""
    import torch
    from pdn_jpegxl_amd import api
    px = synth16(300, 270, 5)
    data = oracle.encode(px, distance=1.0, bits=16)
    ref = oracle.decode(data).pixels
    info = api.peek(data)
    assert info.bytes_per_sample == 2 and info.num_channels == 4
    out = torch.zeros(info.width * info.height * 4 * 2, dtype=torch.uint8, device="cuda")
    dec = api.Decoder(0)
    try:
        assert dec.set_option("no_direct", 1) and dec.set_option("lane_stride", 2)
        st = dec.decode_batch([data], [out.data_ptr()], None, synchronize=True)
        assert st[0] == 0
        assert dec.set_option("query_alpha_narrow_groups", 0) == 0 and dec.set_option("query_alpha_redo_groups", 0) == 0
    finally:
        dec.close()
    got = out.cpu().numpy().view(np.uint16).reshape(info.height, info.width, 4)
    d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    assert d[..., :3].max() <= 48 and (d[..., :3] > 8).mean() < 0.002
    assert np.array_equal(got[..., 3], px[..., 3])
