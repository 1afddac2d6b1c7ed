"""The case table of the asynchronous-pipeline tests, without a GPU: every kind of file takes the path it is in the table for, and
no two outputs that a stale slot or a swapped buffer could confuse hold the same bytes (tests/async_util.py)."""
import numpy as np
import pytest

import async_util as AU
import layer_util as LU
from pdn_jpegxl_amd import api


@pytest.fixture(scope="module")
def table(oracle):
    return AU.table(oracle)


@pytest.fixture(scope="module")
def outputs(oracle, table):
    return [[AU.expected(oracle, c, b.options) for c in b.cases] for b in table]


def test_table_shape(table):
    assert [len(b.cases) for b in table] == [1, 3, 2, 5, 1, 4, 2]
    assert len({tuple(c.kind for c in b.cases) for b in table}) == len(table)          # each batch another selection
    assert len({c.seed for b in table for c in b.cases}) == sum(len(b.cases) for b in table)
    assert {c.kind for b in table for c in b.cases} == set(AU.SIZES)
    assert [b.options for b in table].count({"downscale": 8}) == 1
    assert [b.options for b in table].count({"lane_stride": 2, "no_direct": 1}) == 1
    # a slot that comes round again holds a larger, and later a smaller, layout
    slot0 = [sum(len(c.data) for c in table[k].cases) for k in (0, 3, 6)]
    assert slot0[0] < slot0[1] > slot0[2]
    # 1:8 refuses layered files; the table does not ask for that
    assert all(c.kind not in ("layered", "lossy-noise") for b in table if b.options.get("downscale") == 8 for c in b.cases)


def test_every_kind_takes_its_path(oracle, table):
    seen = set()
    for b in table:
        for c in b.cases:
            st, facts, msg = api.parse_check(c.data)
            assert st == "Ok", (c.kind, msg)
            info = api.peek(c.data)
            assert (info.height, info.width, info.num_channels) == c.shape, c.kind
            assert info.bytes_per_sample == np.dtype(c.dtype).itemsize
            _, h, _ = LU.frame_of(c.data)
            flags = AU.frame_flags(h)
            if c.kind in seen:
                continue
            seen.add(c.kind)
            if c.kind == "lossy-rgba":
                assert h.encoding == 0 and info.num_groups > 1 and info.has_alpha
                first = oracle.decode(c.data, want_dump=True).planes["strategy"]
                first = set((first[first >= 0x80] & 0x7F).tolist())
                assert first & {5, 6, 7, 18, 19, 20}, first          # varblocks of 32 x 32 and more
            elif c.kind == "lossy-one-group":
                assert h.encoding == 0 and info.num_groups == 1 and facts[7] == 1      # one section: the LF pre-pass locates HfGlobal
            elif c.kind in ("lossless-rgb8", "lossless-rgba16"):
                assert h.encoding == 1 and flags == 0 and h.is_last
                assert np.array_equal(oracle.decode(c.data).pixels, c.source)
            elif c.kind == "lossy-noise":
                assert h.encoding == 0 and flags == 1 and h.is_last and info.num_groups > 1
                assert AU.frame_flags(LU.frame_of(c.plain)[1]) == 0
            elif c.kind == "oriented":
                assert h.encoding == 0 and AU.SIZES[c.kind] == (c.shape[0], c.shape[1])   # sides swapped
                assert oracle.decode(c.data).pixels.shape == c.shape
            elif c.kind == "layered":
                assert h.encoding == 1 and not h.is_last and h.crop is None            # a frame follows the first
                assert facts[0] == 0                                                   # the file has no MA tree of its own: its frames do
            elif c.kind == "lossy-u16-pq":
                assert h.encoding == 0 and info.bytes_per_sample == 2 and not info.reserved
    assert seen == set(AU.SIZES)


def test_outputs_that_could_be_confused_differ(table, outputs):
    """Neighbouring batches and batches of one slot: outputs at the same index differ in more than half of their bytes wherever the
    shapes match - and so do any two outputs of the table of one shape, whichever batch and index they have."""
    for b, outs in zip(table, outputs):
        for c, o in zip(b.cases, outs):
            assert o.shape == AU.out_shape(c, b.options) and o.dtype == c.dtype, (b.index, c.kind)
    compared = 0
    flat = [(b.index, k, np.ascontiguousarray(o).view(np.uint8)) for b, outs in zip(table, outputs) for k, o in enumerate(outs)]
    for i, (ba, ka, a) in enumerate(flat):
        for bb, kb, o in flat[i + 1:]:
            if a.shape != o.shape:
                continue
            share = float((a != o).mean())
            assert share > 0.5, (ba, ka, bb, kb, share)
            compared += 1
    assert compared >= 8
    # the pairs the issue names are among them (same index, same shape)
    named = [(a, b, k) for a, b in AU.slot_mates() for k in range(min(len(outputs[a]), len(outputs[b])))
             if outputs[a][k].shape == outputs[b][k].shape and outputs[a][k].dtype == outputs[b][k].dtype]
    assert {(0, 3, 0), (1, 4, 0), (3, 6, 0), (3, 6, 1)} <= set(named), named
