"""CPU tests of the row area of alpha_ans_kernel's one-pass form (csrc/lds_layout.h: AlphaRowsLds): every lane keeps the previous row of
its group as packed u8, 256 bytes a lane, behind the launch's tables - behind the bit windows when the tables stay in global memory.
What the area must look like is written out here on its own; the code shapes and tree sizes are those of tests/test_entropy_plan.py."""
import numpy as np
import pytest

from pdn_jpegxl_amd.synth import synth
from test_entropy_plan import SHAPES, TREES, code_sizes, constants, layout, plan_of

GROUP_DIM = 256


def test_row_area_lies_behind_the_tables():
    c = constants()
    for shape in SHAPES:
        for nodes in TREES:
            for slots in (1, 8, 32, 64):
                windows = slots * c["ring_words"] * 4
                tables_end, rows, end, host, g_rows, g_end = layout(6, slots, nodes, *shape)
                # the tables as test_lf_and_alpha_layout knows them: windows | tree | alias | cfg | cmap
                assert tables_end == layout(2, slots, nodes, *shape)[5]
                assert tables_end >= windows + 16 * nodes + sum(code_sizes(shape))
                # behind them, on a dword, no further than that asks, one group row of bytes per lane
                assert rows % 4 == 0 and tables_end <= rows < tables_end + 4
                assert end == rows + slots * GROUP_DIM
                # inside what the host asks for, which is the tables' bytes and the rows' and no more
                assert end <= host == layout(2, slots, nodes, *shape)[6] + slots * GROUP_DIM
                # tables in global memory: straight behind the windows
                assert g_rows == windows and g_end == windows + slots * GROUP_DIM


@pytest.fixture(scope="module")
def rgba_files(oracle):
    return {size: oracle.encode(synth(size[0], size[1], 41), distance=1.0) for size in ((528, 264), (272, 17))}


@pytest.mark.parametrize("stride", [1, 2, 8])
def test_a_lane_path_plan_holds_the_row_area(rgba_files, stride):
    files = list(rgba_files.values())
    P = plan_of(files, lane_stride=stride, no_direct=True)
    slots = 64 // stride
    assert P["per_alpha_wg"] == slots and not P["direct_alpha"] and not P["alpha_global"]
    for f in P["frames"]:
        tables_end, rows, end, host, _, _ = layout(6, slots, f["tree_nodes"], *f["mcode"])
        assert end <= P["lds_alpha"]
    # and no more than the largest frame's tables and rows
    assert P["lds_alpha"] == max(layout(6, slots, f["tree_nodes"], *f["mcode"])[3] for f in P["frames"])
    assert P["lds_alpha"] - max(layout(2, slots, f["tree_nodes"], *f["mcode"])[6] for f in P["frames"]) == slots * GROUP_DIM
    # the LF launch shares SlotsLds and keeps its size
    assert P["lds_lf"] == max(layout(2, P["lf_per_wave"], f["tree_nodes"], *f["mcode"])[6] for f in P["frames"])


def test_a_direct_alpha_plan_is_unchanged(rgba_files):
    """One section per wavefront on the scalar unit: two passes, no row area."""
    files = list(rgba_files.values())
    P = plan_of(files)
    assert P["direct_alpha"] and P["per_alpha_wg"] == 1
    assert P["lds_alpha"] == max(layout(2, 1, f["tree_nodes"], *f["mcode"])[6] for f in P["frames"])
