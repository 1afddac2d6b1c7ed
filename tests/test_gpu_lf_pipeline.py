"""The LF channels' prediction pass as a register pipeline (lf_finish_gradient_kernel) against the oracle and against the row-per-lane
pass it replaces (option no_lf_pipeline), on the smallest frames at which its schedule can go wrong.

The oracle writes all three LF channels with the gradient predictor, so every frame here takes the pipeline.  Each case checks the
stage taps and the pixels against the oracle the way test_gpu_parity.run_case does (same tolerances, imported from there), then
decodes the same bytes with no_lf_pipeline = 1 and requires the three quantised LF planes and the output bytes to be identical.
"""
import numpy as np
import pytest

from pdn_jpegxl_amd.synth import synth
from gpu_helpers import compare_stages, gpu_decode
from test_gpu_parity import check_pixels, check_report

pytestmark = pytest.mark.gpu


def lf_planes(dec, index):
    return [dec.read_plane(index, "lf_quant", c).copy() for c in range(3)]


def both_forms(dec, oracle, files):
    """Decodes `files` as one batch with the pipeline and without it; every frame against the oracle, the two forms against each other."""
    dumps = [oracle.decode(f, want_dump=True) for f in files]
    assert dec.set_option("no_lf_pipeline", 0)
    outs = gpu_decode(dec, files, taps=True)
    lfq = []
    for i, (out, od) in enumerate(zip(outs, dumps)):
        check_report(compare_stages(dec, i, od))
        check_pixels(out, od.pixels)
        lfq.append(lf_planes(dec, i))
    assert dec.set_option("no_lf_pipeline", 1)
    try:
        old = gpu_decode(dec, files, taps=True)
        for i, (out, o) in enumerate(zip(outs, old)):
            for c, (a, b) in enumerate(zip(lfq[i], lf_planes(dec, i))):
                assert a.shape == b.shape and (a == b).all(), (i, c)
            assert out.tobytes() == o.tobytes(), i
    finally:
        dec.set_option("no_lf_pipeline", 0)
    return dumps


def layout_of(img, layout):
    return np.ascontiguousarray({"rgba": img, "rgb": img[..., :3], "gray": img[..., 1:2]}[layout])


# (width, height) in pixels -> cells w8 x h8
SHAPES = [
    (128, 8),      # 16 x 1: one row, top-row rule only
    (128, 136),    # 16 x 17: row 16 wraps from lane 15 back to lane 0
    (256, 264),    # 32 x 33: two lines per row (the carried North-West), third block of rows
    (2048, 24),    # 256 x 3: sixteen lines per row, a lane goes from one row straight to its next
    (2176, 136),   # 272 x 17: two LF groups side by side, 256 and 16 cells wide
    (128, 2176),   # 16 x 272: two LF groups stacked, 256 and 16 rows
    (136, 40),     # 17 x 5: partial last line; stride not a multiple of four
    (120, 40),     # 15 x 5: partial last line; stride not a multiple of four
    (600, 400),    # 75 x 50: partial last line; stride not a multiple of four
    (8, 8),        # 1 x 1: one cell
]


@pytest.mark.parametrize("size", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_shapes(gpu_decoder, oracle, size):
    (od,) = both_forms(gpu_decoder, oracle, [oracle.encode(synth(size[0], size[1], 31))])
    assert (od.w8, od.h8) == ((size[0] + 7) // 8, (size[1] + 7) // 8)


@pytest.mark.parametrize("layout", ["gray", "rgb", "rgba"])
def test_channel_layouts(gpu_decoder, oracle, layout):
    both_forms(gpu_decoder, oracle, [oracle.encode(layout_of(synth(256, 264, 32), layout))])


def test_different_group_shapes_in_one_launch(gpu_decoder, oracle):
    """One batch, one launch of each LF kernel: every wavefront has its own group shape and loop bound."""
    imgs = [synth(128, 136, 33), synth(2176, 136, 34), synth(600, 400, 35), layout_of(synth(256, 264, 36), "gray")]
    both_forms(gpu_decoder, oracle, [oracle.encode(im) for im in imgs])


@pytest.mark.parametrize("enc", [dict(num_passes=2), dict(lf_contexts=True)], ids=["two-passes", "lf-contexts"])
def test_progressive_and_lf_contexts(gpu_decoder, oracle, enc):
    """hf_blocklist_kernel reads the quantised LF for the block contexts' thresholds: the planes must be final when it runs."""
    both_forms(gpu_decoder, oracle, [oracle.encode(synth(256, 264, 37), **enc)])
