"""Alpha in one pass: alpha_ans_kernel's lane path applies the clamped gradient itself (West in a register, North / North-West from the
lane's previous row kept as packed u8 in LDS) and stores sixteen finished u8 samples at a time to the alpha plane; there is no residual
plane and no second pass for such a group.

Frames are oracle.encode(image, distance=1.0) of synth(w, h, 41) with its alpha kept or replaced.  Every case asks for the bench's
launch shape (no_direct = 1, lane_stride = 2) unless it varies it, and checks

  * alpha equal to the source exactly,
  * colour through check_pixels against the oracle's decode,
  * bytes identical to the same decode with alpha_narrow_limit = 0 (int32 residuals, two passes: the form every group had before),

and the counters: query_alpha_narrow_groups counts the groups finished in one pass, query_alpha_redo_groups those the lane gave up
(a residual above alpha_narrow_limit, or a finished sample outside 0 .. alpha_sample_limit) and the redo launch decoded again.

Eligible (test_gpu_alpha_narrow.eligible_groups): a group alpha_ans_kernel decodes (a frame of more than one group; a one-group frame has
its alpha in LfGlobal) whose width is a multiple of 16 in a frame whose width is a multiple of 4, 8-bit alpha, every row a gradient leaf
(what the oracle writes) and no row of one-symbol tokens.
"""
import numpy as np
import pytest

from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth, synth16
from test_gpu_alpha_narrow import eligible_groups
from test_gpu_parity import check_pixels

pytestmark = pytest.mark.gpu

# more than one group each: 272x1 top-row rule only; 272x264 a second group row (first-column and North rules across the row buffer's
# reuse); 1040x17 a last group 16 wide (one line per row)
SHAPES = [(272, 1), (272, 17), (528, 2), (272, 264), (1040, 17), (528, 264)]
CONTENTS = ["synth", "random", "checker"]

_cache = {}


def image(size, content):
    w, h = size
    img = synth(w, h, 41).copy()
    if content == "random":     # both clamp branches and large residuals
        img[..., 3] = np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w), dtype=np.uint8)
    elif content == "checker":  # 0 / 255 in cells of 3 x 5: the extremes beside each other
        yy, xx = np.mgrid[0:h, 0:w]
        img[..., 3] = np.where(((xx // 3) + (yy // 5)) & 1, 255, 0).astype(np.uint8)
    elif content == "constant":  # every gradient residual is 0: one-symbol tokens in every row
        img[..., 3] = 0
    elif content == "opaque":
        img = np.ascontiguousarray(img[..., :3])
    else:
        assert content == "synth"
    return img


def frame(oracle, size, content="synth"):
    """(source, file, oracle's pixels), encoded and decoded by the oracle once for the whole module."""
    key = (size, content)
    if key not in _cache:
        img = image(size, content)
        data = oracle.encode(img, distance=1.0)
        _cache[key] = (img, data, oracle.decode(data).pixels)
    return _cache[key]


def decode(dec, files, narrow_limit=32767, sample_limit=255, lane_stride=2, band=None):
    """One batch on the lane path; returns (output bytes per image as uint8 arrays, groups finished in one pass, groups decoded again)."""
    import torch
    infos = [api.peek(f) for f in files]
    rows = [i.height for i in infos]
    if band:
        rows = [min(i.height, (band[0] + band[1]) * 256) - min(i.height, band[0] * 256) for i in infos]
    outs = [torch.zeros(r * i.width * i.num_channels * i.bytes_per_sample, dtype=torch.uint8, device="cuda") for r, i in zip(rows, infos)]
    assert dec.set_option("no_direct", 1) and dec.set_option("lane_stride", lane_stride)
    assert dec.set_option("alpha_narrow_limit", narrow_limit) and dec.set_option("alpha_sample_limit", sample_limit)
    if band:
        assert dec.set_option("band_first_row", band[0]) and dec.set_option("band_rows", band[1])
    try:
        st = dec.decode_batch(files, [o.data_ptr() for o in outs], None, synchronize=True)
        assert all(s == 0 for s in st), st
        counts = dec.set_option("query_alpha_narrow_groups", 0), dec.set_option("query_alpha_redo_groups", 0)
    finally:
        dec.set_option("no_direct", 0)
        dec.set_option("lane_stride", 0)
        dec.set_option("alpha_narrow_limit", 32767)
        dec.set_option("alpha_sample_limit", 255)
        dec.set_option("band_rows", 0)
        dec.set_option("band_first_row", 0)
    return [o.cpu().numpy() for o in outs], counts[0], counts[1]


def as_pixels(raw, img):
    return raw.reshape(img.shape)


def check_frame(raw, fr):
    img, _, ref = fr
    out = as_pixels(raw, img)
    if img.shape[2] == 4:
        assert (out[..., 3] == img[..., 3]).all(), int((out[..., 3] != img[..., 3]).sum())
    check_pixels(out, ref)


def same_bytes(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.tobytes() == y.tobytes(), (i, int((x != y).sum()))


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("size", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_shapes_and_contents(gpu_decoder, oracle, size, content):
    fr = frame(oracle, size, content)
    eligible = eligible_groups(*size)
    assert eligible > 0
    outs, narrow, redo = decode(gpu_decoder, [fr[1]])
    two_pass, n0, r0 = decode(gpu_decoder, [fr[1]], narrow_limit=0)
    print("%s %s: eligible %d, one pass %d, redo %d; limit 0: %d, %d" % (size, content, eligible, narrow, redo, n0, r0))
    check_frame(outs[0], fr)
    same_bytes(outs, two_pass)
    assert (narrow, redo) == (eligible, 0)
    assert (n0, r0) == (0, 0)


@pytest.mark.parametrize("narrow_limit", [32767, 100])
@pytest.mark.parametrize("size", [(528, 264), (1040, 17)], ids=["528x264", "1040x17"])
def test_a_sample_out_of_range_gives_the_group_up(gpu_decoder, oracle, size, narrow_limit):
    """synth's alpha is 64 .. 255: with alpha_sample_limit = 200 a lane that meets a larger sample stops, and the redo launch decodes
    its group as int32.  Together with alpha_narrow_limit = 100 both conditions give groups up."""
    fr = frame(oracle, size)
    assert fr[0][..., 3].max() > 200
    eligible = eligible_groups(*size)
    default, narrow_d, redo_d = decode(gpu_decoder, [fr[1]])
    assert (narrow_d, redo_d) == (eligible, 0)
    outs, narrow, redo = decode(gpu_decoder, [fr[1]], narrow_limit=narrow_limit, sample_limit=200)
    print("%s narrow limit %d sample limit 200: eligible %d, one pass %d, redo %d" % (size, narrow_limit, eligible, narrow, redo))
    assert narrow + redo == eligible and redo > 0
    check_frame(outs[0], fr)
    same_bytes(outs, default)


def test_lane_strides(gpu_decoder, oracle):
    """64, 32, 16 and 8 lanes per wavefront: the row area is indexed by the launch's slots."""
    size = (528, 264)
    fr = frame(oracle, size)
    first = None
    for stride in (1, 2, 4, 8):
        outs, narrow, redo = decode(gpu_decoder, [fr[1]], lane_stride=stride)
        assert (narrow, redo) == (eligible_groups(*size), 0), stride
        if first is None:
            first = outs
            check_frame(outs[0], fr)
        else:
            same_bytes(outs, first)
    same_bytes(decode(gpu_decoder, [fr[1]], narrow_limit=0)[0], first)


def test_different_frames_in_one_launch(gpu_decoder, oracle):
    """An eligible frame, constant alpha (rows of one-symbol tokens: two passes, counted nowhere), a one-group frame, a frame without
    alpha and a 16-bit-alpha frame in one launch of each alpha kernel."""
    frames = [frame(oracle, (528, 264)), frame(oracle, (272, 264), "constant"), frame(oracle, (24, 40)), frame(oracle, (272, 17), "opaque")]
    px16 = synth16(300, 270, 5)
    data16 = oracle.encode(px16, distance=1.0, bits=16)
    info = api.peek(data16)
    assert info.bytes_per_sample == 2 and info.num_channels == 4
    files = [f[1] for f in frames] + [data16]
    outs, narrow, redo = decode(gpu_decoder, files)
    two_pass, n0, r0 = decode(gpu_decoder, files, narrow_limit=0)
    print("mixed launch: one pass %d, redo %d; limit 0: %d, %d" % (narrow, redo, n0, r0))
    assert (narrow, redo) == (eligible_groups(528, 264), 0) and (n0, r0) == (0, 0)
    same_bytes(outs, two_pass)
    for raw, fr in zip(outs, frames):
        check_frame(raw, fr)
    got16 = outs[4].view(np.uint16).reshape(info.height, info.width, 4)
    assert np.array_equal(got16[..., 3], px16[..., 3])
    # each frame alone decodes to the same bytes; the constant one is counted nowhere
    for i in (0, 1):
        alone, narrow, redo = decode(gpu_decoder, [files[i]])
        same_bytes(alone, [outs[i]])
        assert (narrow, redo) == ((eligible_groups(528, 264), 0) if i == 0 else (0, 0))


def test_two_contents_of_one_size_one_after_the_other(gpu_decoder, oracle):
    """Nothing of the previous batch's planes or row buffers shows in the next."""
    size = (528, 264)
    a, b = frame(oracle, size, "random"), frame(oracle, size, "checker")
    got = []
    for fr in (a, b, a):
        outs, narrow, redo = decode(gpu_decoder, [fr[1]])
        assert (narrow, redo) == (eligible_groups(*size), 0)
        check_frame(outs[0], fr)
        got.append(outs)
    for fr, outs in zip((a, b, a), got):
        same_bytes(outs, decode(gpu_decoder, [fr[1]], narrow_limit=0)[0])


def test_band_decode(gpu_decoder, oracle):
    """272 x 776 is four group rows; the band of rows 1 .. 2 equals those rows of the whole decode."""
    size = (272, 776)
    fr = frame(oracle, size)
    whole, narrow, redo = decode(gpu_decoder, [fr[1]])
    assert (narrow, redo) == (eligible_groups(*size), 0)
    check_frame(whole[0], fr)
    band, narrow, redo = decode(gpu_decoder, [fr[1]], band=(1, 2))
    assert (narrow, redo) == (2 * 2, 0)   # two group rows of two groups
    rows = as_pixels(whole[0], fr[0])[256:768]
    assert band[0].tobytes() == rows.tobytes(), int((band[0].reshape(rows.shape) != rows).sum())
    same_bytes(decode(gpu_decoder, [fr[1]], narrow_limit=0, band=(1, 2))[0], band)
