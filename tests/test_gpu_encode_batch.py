"""GPU tests of the batch encoder (include/jxlfiletypeio.h, Part 4: jxlhip_encoder_* / jxlhip_encode_batch).

The one rule: the file of every image of a batch is, byte for byte, the file jxlhip_save_pixels writes for the same pixels (in host
memory), options and metadata.  The shapes are the smallest that reach each path of the batch kernels: 1 x 1, 8 x 8 and 9 x 9 (one cell,
padded edges), 256 x 256 RGBA (one group: alpha in the global section), 264 x 200 RGBA (two ragged groups, alpha in the pass groups),
2056 x 16 (two LF groups, nine groups).  The references are computed once per module and never changed."""
import numpy as np
import pytest
import torch

from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth
from save_pixels_util import channels, float_image, u16_image

pytestmark = pytest.mark.gpu


class Spec:
    """One image: its samples (numpy, host) and how it is encoded - by save_pixels for the reference, by the batch for the test."""

    def __init__(self, px, bits=None, **kw):
        self.px, self.bits, self.kw = px, bits, kw

    def reference(self):
        return api.save_pixels(self.px, bits=self.bits, **self.kw)

    def item(self, pitch_extra=0):
        """The samples in device memory (rows `pitch_extra` bytes further apart than they need be) as an EncodeItem."""
        h, w, c = self.px.shape
        row = w * c * self.px.dtype.itemsize
        host = np.zeros((h, row + pitch_extra), np.uint8)
        host[:, :row] = np.ascontiguousarray(self.px).view(np.uint8).reshape(h, row)
        dev = torch.from_numpy(host).cuda()
        return api.EncodeItem(dev.data_ptr(), w, h, c, self.px.dtype, stride_bytes=row + pitch_extra, bits=self.bits, keep=dev, **self.kw)


def u8(w, h, seed, nch):
    return channels(synth(w, h, seed), nch)


def lossy_specs():
    return [
        Spec(u8(1, 1, 1, 1), distance=1.0, effort=7),
        Spec(u8(8, 8, 2, 2), distance=0.5, effort=1),
        Spec(u16_image(9, 9, 3, 10, 3), bits=10, distance=1.0, effort=5, colour="DisplayP3"),
        Spec(u8(256, 256, 4, 4), distance=1.0, effort=7),
        Spec(u16_image(264, 200, 5, 16, 4), bits=16, distance=4.5, effort=7),
        Spec(u8(2056, 16, 6, 3), distance=1.0, effort=5),
        Spec(float_image(264, 200, 7, np.float16, 4), distance=0.5, effort=7, colour="Rec2020Linear"),
        Spec(float_image(9, 9, 8, np.float32, 4), distance=1.0, effort=1, colour="Rec2020PQ"),
        Spec(u16_image(256, 256, 9, 16, 2), bits=16, distance=4.5, effort=5, colour="LinearGray"),
        Spec(u8(2056, 16, 10, 4), distance=0.5, effort=7),
        Spec(float_image(264, 200, 11, np.float32, 3), distance=1.0, effort=5, colour="LinearSrgb"),
    ]


def lossless_specs():
    out = []
    sizes = [(9, 9), (256, 256), (264, 200), (2056, 16)]
    for nch in (1, 2, 3, 4):
        w, h = sizes[nch - 1]
        out.append(Spec(u8(w, h, 20 + nch, nch), lossless=True, effort=1 if nch & 1 else 7))
        w, h = sizes[(nch + 1) % 4]
        out.append(Spec(u16_image(w, h, 30 + nch, 12 if nch == 2 else 16, nch), bits=12 if nch == 2 else 16, lossless=True, effort=7 if nch & 1 else 1))
    return out


@pytest.fixture(scope="module")
def encoder():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the product path has no CPU fallback")
    enc = api.Encoder(0)
    yield enc
    enc.close()


@pytest.fixture(scope="module")
def lossy():
    specs = lossy_specs()
    return specs, [s.item() for s in specs], [s.reference() for s in specs]


@pytest.fixture(scope="module")
def lossless():
    specs = lossless_specs()
    return specs, [s.item() for s in specs], [s.reference() for s in specs]


def same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g is not None, "image %d has no result" % i
        assert g == w, "image %d: %d bytes against %d of save_pixels" % (i, len(g), len(w))


# ---------------------------------------------------------------- 1. lossy
def test_mixed_lossy_batch_writes_the_bytes_of_save_pixels(encoder, lossy):
    specs, items, refs = lossy
    assert {s.kw["effort"] for s in specs} == {1, 5, 7} and {s.kw["distance"] for s in specs} == {0.5, 1.0, 4.5}
    same(encoder.encode_batch(items), refs)
    assert encoder.last_statuses == ["Ok"] * len(items)


def test_the_same_batch_again_and_in_reverse_writes_the_same_bytes(encoder, lossy):
    _, items, refs = lossy
    same(encoder.encode_batch(items), refs)                  # the workspace is reused, its counters cleared
    same(encoder.encode_batch(items[::-1]), refs[::-1])      # every image at another place of the workspace and of the grids
    same(encoder.encode_batch(items), refs)


# ---------------------------------------------------------------- 2. lossless
def test_lossless_integers_beside_lossy_images_write_the_bytes_of_save_pixels(encoder, lossy, lossless):
    _, ll_items, ll_refs = lossless
    _, lossy_items, lossy_refs = lossy
    items = [lossy_items[4]] + ll_items[:4] + [lossy_items[3]] + ll_items[4:] + [lossy_items[9]]
    refs = [lossy_refs[4]] + ll_refs[:4] + [lossy_refs[3]] + ll_refs[4:] + [lossy_refs[9]]
    same(encoder.encode_batch(items), refs)


def test_a_lossless_result_decodes_to_its_source(encoder, lossless):
    specs, items, _ = lossless
    k = next(i for i, s in enumerate(specs) if s.px.dtype == np.uint16 and s.bits == 16 and s.px.shape[2] == 4)
    data = encoder.encode_batch([items[k]])[0]
    got = api.load_image(data)
    assert got.channel_representation == 1 and np.array_equal(got.pixels, specs[k].px)


# ---------------------------------------------------------------- 3. batch sizes and group counts
def test_batch_of_one(encoder, lossy):
    _, items, refs = lossy
    for k in (0, 3, 9):
        same(encoder.encode_batch([items[k]]), [refs[k]])


def test_images_that_all_differ_in_their_group_count(encoder):
    sizes = [(40, 30), (264, 200), (600, 100), (300, 280), (2056, 16), (520, 300)]   # 1, 2, 3, 4, 9 and 6 groups
    assert len({((w + 255) // 256) * ((h + 255) // 256) for w, h in sizes}) == len(sizes)
    specs = [Spec(u8(w, h, 40 + i, 4), distance=1.0, effort=7) for i, (w, h) in enumerate(sizes)]
    same(encoder.encode_batch([s.item() for s in specs]), [s.reference() for s in specs])


# ---------------------------------------------------------------- 4. strided input
def test_strided_device_rows_equal_tight_rows(encoder, lossy, lossless):
    picks = [(lossy, 4), (lossy, 5), (lossy, 10), (lossless, 1), (lossless, 6)]
    items = [case[0][k].item(pitch_extra=24 if case[0][k].px.dtype.itemsize > 1 else 13) for case, k in picks]
    assert all(it.stride_bytes > it.width * it.channels * it.dtype.itemsize for it in items)
    same(encoder.encode_batch(items), [case[2][k] for case, k in picks])


# ---------------------------------------------------------------- 5. metadata
def test_exif_and_xmp_on_one_image_of_a_batch(encoder, lossy):
    specs, items, refs = lossy
    exif = b"\0\0\0\0II*\0\x08\0\0\0\0\0\0\0\0\0"
    xmp = b"<x:xmpmeta xmlns:x='adobe:ns:meta/'></x:xmpmeta>"
    with_md = Spec(specs[4].px, bits=specs[4].bits, exif=exif, xmp=xmp, **specs[4].kw)
    want = with_md.reference()
    assert want != refs[4] and exif[4:] in want and xmp in want
    same(encoder.encode_batch([items[3], with_md.item(), items[5]]), [refs[3], want, refs[5]])


# ---------------------------------------------------------------- 6. refusals
def test_refused_images_leave_their_neighbours_alone(encoder, lossy):
    specs, items, refs = lossy
    effort8 = Spec(specs[3].px, distance=1.0, effort=8).item()
    ll_float = Spec(specs[7].px, lossless=True, effort=7).item()
    with_icc = Spec(specs[3].px, distance=1.0, effort=7).item()
    with_icc.icc = b"\0" * 128
    five = Spec(specs[3].px, distance=1.0, effort=7).item()
    five.channels = 5
    batch = [items[3], effort8, items[4], ll_float, with_icc, items[9], five]
    got = encoder.encode_batch(batch, raise_on_error=False)
    assert encoder.last_statuses == ["Ok", "EncodeError", "Ok", "EncodeError", "EncodeError", "Ok", "EncodeError"]
    assert encoder.last_error.startswith("image 1: ") and "efforts 8 and 9" in encoder.last_error
    assert [g is None for g in got] == [False, True, False, True, True, False, True]
    same([got[0], got[2], got[5]], [refs[3], refs[4], refs[9]])
    for bad, text in ((ll_float, "lossless float"), (with_icc, "ICC"), (five, "number of channels")):
        with pytest.raises(api.JxlError) as e:
            encoder.encode_batch([bad])
        assert e.value.status == "EncodeError" and "image 0: " in str(e.value) and text in str(e.value)
    same(encoder.encode_batch([items[3], items[4]]), [refs[3], refs[4]])   # the encoder goes on working


def test_empty_batch(encoder):
    assert encoder.encode_batch([]) == [] and encoder.last_statuses == []
    assert encoder.stage_times() == {}


# ---------------------------------------------------------------- 7. stage times
def test_stage_times_name_the_reverse_stages_and_a_warm_call_allocates_nothing(encoder, lossy):
    _, items, refs = lossy
    same(encoder.encode_batch(items), refs)
    same(encoder.encode_batch(items), refs)
    st = encoder.stage_times()
    reverse = [k for k in st if k.startswith("reverse pass")]
    assert len(reverse) == 2 and all("one launch" in k for k in reverse)
    assert any(k.startswith("section bit layout") for k in st) and any(k.startswith("compaction") for k in st)
    assert any(k.startswith("host: HF code construction") for k in st) and "host: assembly" in st
    assert not [k for k in st if "allocation" in k]
    assert all(v >= 0 for v in st.values())


def test_a_fresh_encoder_reports_its_allocations(lossy):
    _, items, refs = lossy
    enc = api.Encoder(0)
    try:
        same(enc.encode_batch(items[:2]), refs[:2])
        assert "host: workspace allocation" in enc.stage_times()
    finally:
        enc.close()
