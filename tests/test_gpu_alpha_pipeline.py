"""The alpha plane's prediction pass as a register pipeline (alpha_finish_gradient_kernel) on the smallest frames at which its schedule
can go wrong, and on widths it leaves to alpha_finish_kernel.

The oracle writes the alpha channel of a lossy frame losslessly with one gradient leaf, so every group whose width is a multiple of 16
takes the pipeline.  The decoded alpha must be the source's alpha exactly; the colour samples are checked against the oracle's decode
the way test_gpu_parity does.
"""
import pytest

from pdn_jpegxl_amd.synth import synth
from gpu_helpers import gpu_decode
from test_gpu_parity import check_pixels

pytestmark = pytest.mark.gpu


def decode_and_check(dec, oracle, sizes):
    """Encodes RGBA synth(w, h, 41) for every (w, h), decodes them as one batch, checks alpha against the source and pixels against the oracle."""
    imgs = [synth(w, h, 41) for w, h in sizes]
    files = [oracle.encode(img, distance=1.0) for img in imgs]
    for img, out, data in zip(imgs, gpu_decode(dec, files), files):
        assert out.shape == img.shape
        assert (out[..., 3] == img[..., 3]).all()
        check_pixels(out, oracle.decode(data).pixels)


# (width, height) in pixels; an alpha group is 256 x 256, sixteen lanes own a group, four groups share a wavefront
SHAPES = [
    (16, 1),       # one line, one row: top-row rule only
    (16, 17),      # row 16 wraps from lane 15 back to lane 0
    (32, 33),      # two lines per row (the carried North-West), third block of rows
    (256, 3),      # sixteen lines per row: a lane goes from one row straight to its next
    (272, 17),     # two groups side by side, 256 and 16 wide, in one wavefront with different line counts
    (16, 272),     # two groups stacked, 256 and 16 rows
    (1040, 17),    # five groups: a second wavefront with one live team
    (528, 264),    # four groups of different shapes in one wavefront
    (24, 40),      # width not a multiple of 16: left to alpha_finish_kernel
    (20, 9),       # likewise
]


@pytest.mark.parametrize("size", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_shapes(gpu_decoder, oracle, size):
    decode_and_check(gpu_decoder, oracle, [size])


def test_different_frames_in_one_launch(gpu_decoder, oracle):
    """One batch, one launch of each alpha kernel: frames the pipeline takes beside one it leaves alone."""
    decode_and_check(gpu_decoder, oracle, [(16, 17), (272, 17), (24, 40), (528, 264)])
