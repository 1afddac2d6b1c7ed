"""Modular transform lists on the GPU: every reversible colour transform, transforms at channel offsets, chains across the switch
from the inline route (RCTs undone inside modular_out_kernel) to the launch route (rct_inverse_kernel, unsqueeze_h_kernel,
unsqueeze_v_kernel, palette_inverse_kernel), explicit Squeeze lists down to channels without samples, and palettes over part of the
channels.  The streams are those of tests/transform_util.py's case table, which tests/test_transform_chains.py holds against a
numpy restatement on the CPU.

The bar: every decoded sample equals the source and the oracle's decode - no tolerance, nothing excluded.  Each group is decoded as
one batch (frames with different transform tables side by side); a handful of streams are decoded alone as well and must be
byte-identical to their batch entry."""
import numpy as np
import pytest

import downscale_util as DU
import layer_util as LU
import transform_util as TU
from pdn_jpegxl_amd import api

pytestmark = pytest.mark.gpu


def decode_batch(dec, files):
    """One decode_batch of the files -> arrays (h, w, channels) of each file's own sample type."""
    import torch
    infos = [api.peek(f) for f in files]
    outs = [torch.empty(i.width * i.height * i.num_channels * i.bytes_per_sample, dtype=torch.uint8, device="cuda") for i in infos]
    torch.cuda.synchronize()
    st = dec.decode_batch(files, [o.data_ptr() for o in outs])
    assert all(s == 0 for s in st), st
    return [o.cpu().numpy().view(DU.dtype_of(i)).reshape(i.height, i.width, i.num_channels) for o, i in zip(outs, infos)]


@pytest.fixture(scope="module")
def streams(oracle):
    """name -> (file, the oracle's pixels), encoded and decoded once."""
    memo = {}

    def get(case):
        if case.name not in memo:
            data = case.encode(oracle)
            memo[case.name] = (data, oracle.decode(data).pixels)
        return memo[case.name]
    return get


def check_group(dec, streams, cases):
    files = [streams(c)[0] for c in cases]
    outs = decode_batch(dec, files)
    bad = []
    for c, out in zip(cases, outs):
        want = c.expected()
        assert out.dtype == want.dtype and out.shape == want.shape, (c.name, out.dtype, out.shape)
        if not (np.array_equal(out, want) and np.array_equal(out, streams(c)[1])):
            bad.append("%s (%s, %d samples off)" % (c.name, c.route, int((out != want).sum())))
    assert not bad, "%d of %d cases differ: %s" % (len(bad), len(cases), "; ".join(bad))
    return outs


@pytest.mark.parametrize("route", ["inline", "launches"])
def test_every_rct_type(gpu_decoder, streams, route):
    """a. inline: the 42 types alone; launches: each before the default Squeeze, four of them before a Palette."""
    cases = [c for c in TU.cases_of("a") if c.route == route]
    assert len(cases) == (42 if route == "inline" else 46)
    check_group(gpu_decoder, streams, cases)


def test_offsets_and_depths(gpu_decoder, streams):
    """b. RCTs over G, B, A; the 16-bit range's largest steps; the fifth entry of the inline register array (C, M, Y, K, A)."""
    cases = TU.cases_of("b")
    assert {c.src.shape[2] for c in cases} == {3, 4, 5} and {c.bits for c in cases} == {8, 16}
    check_group(gpu_decoder, streams, cases)


def test_chains_across_the_route_switch(gpu_decoder, streams):
    """c. two and four RCTs inline, the same list with a fifth through launches, a type twice, a chain before the default Squeeze."""
    check_group(gpu_decoder, streams, TU.cases_of("c"))


def test_explicit_squeeze_lists(gpu_decoder, streams):
    """d. single steps, residuals in place and at the end of the list, chroma only, two Squeeze transforms, an RCT over averages and
    over residuals, channels squeezed down to one sample and past it, the 1-wide frames whose empty residuals end the global stream."""
    cases = TU.cases_of("d")
    assert sum(c.zero_size for c in cases) >= 3
    check_group(gpu_decoder, streams, cases)


def test_partial_and_repeated_palettes(gpu_decoder, streams):
    """e. palettes over alpha or colour only, two palettes, a squeezed index channel, colour counts at the size field's edges."""
    check_group(gpu_decoder, streams, TU.cases_of("e"))


ALONE = ["rct23", "rct41+squeeze", "rct13+palette", "cmyka-rct20@2", "chain4", "chain5", "5x3-to-nothing", "1x300-default", "two-palettes"]


def test_alone_equals_batch_entry(gpu_decoder, streams):
    """The named streams, one decode_batch each, against their entry in a batch of every case of the table."""
    batch = dict(zip((c.name for c in TU.CASES), check_group(gpu_decoder, streams, TU.CASES)))
    by = {c.name: c for c in TU.CASES}
    for name in ALONE:
        alone = decode_batch(gpu_decoder, [streams(by[name])[0]])[0]
        assert alone.tobytes() == batch[name].tobytes(), name


# ---------------------------------------------------------------- f. downstream consumers
def test_reduced_size_decode(gpu_decoder, streams):
    """1:8 of a Modular frame is the cell mean of its full-size samples: the inverse transforms run first."""
    cases = TU.cases_of("f")
    assert len(cases) == 2
    st, imgs = DU.decode_reduced_batch(gpu_decoder, [streams(c)[0] for c in cases])
    assert st == [0, 0], (st, gpu_decoder.last_error)
    for c, img in zip(cases, imgs):
        assert np.array_equal(img, DU.box_mean_int(c.src)), c.name


def test_bottom_frame_of_a_layered_file(oracle):
    """The transformed frame under a kReplace layer: the composite is the source with the layer's pixels put in."""
    for i, c in enumerate(TU.cases_of("f")):
        h, w = c.src.shape[:2]
        patch = TU.rgba8(10, 6, 430 + i)
        x0, y0 = 5 + i, 7
        bottom = c.encode(oracle, container=False)
        top = oracle.encode(patch, lossless=True, container=False)
        got = api.load_image(LU.layered(bottom, [LU.Layer(bottom, crop=False), LU.Layer(top, x0=x0, y0=y0)])).pixels
        want = c.src.copy()
        want[y0:y0 + 6, x0:x0 + 10] = patch
        assert got.shape == want.shape and np.array_equal(got, want), c.name


# ---------------------------------------------------------------- g. refusals
@pytest.mark.parametrize("name,picture,transforms", TU.REFUSALS, ids=[r[0] for r in TU.REFUSALS])
def test_invalid_transform_entries_are_refused(oracle, name, picture, transforms):
    """One stream per load_image call: an error with a message, never an image."""
    data = oracle.encode(picture(), lossless=True, transforms=transforms)
    with pytest.raises(api.JxlError) as e:
        api.load_image(data)
    assert len(str(e.value)) > len(e.value.status) + 2, str(e.value)
    # the same picture under the list without the declared entry decodes
    src = picture()
    got = api.load_image(oracle.encode(src, lossless=True, transforms=transforms[:-1])).pixels
    assert np.array_equal(got, src)
