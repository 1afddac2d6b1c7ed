"""CPU tests of the host pieces of the lossless efforts 8 and 9 (DESIGN.md §2 "Lossless efforts 8 and 9"): the searched MA tree as the
writer serialises it, and whole one-group files written by the host pieces alone (palette header; the effort-9 tree), parsed by the
product's host parser and decoded by the oracle.  The entry points live in the self-test library, as the writer self tests do."""
import ctypes as C

import numpy as np
import pytest

from pdn_jpegxl_amd import api


def _lib():
    L = api.selftest_lib()
    L.jxlhip_selftest_lossless_tree.restype = C.c_int32
    L.jxlhip_selftest_lossless_tree.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(api.ErrorInfo)]
    L.jxlhip_selftest_lossless_file.restype = C.c_size_t
    L.jxlhip_selftest_lossless_file.argtypes = [C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t]
    return L


@pytest.mark.parametrize("nch,preds,wp_ctx,palette", [
    (1, [5], 0, 0), (2, [1, 4], 0, 0), (3, [2, 3, 5], 0, 0), (4, [5, 1, 2, 4], 0, 0),        # effort 8: one leaf per channel
    (1, [6], 1, 0), (2, [6, 5], 1, 0), (3, [6, 6, 1], 1, 0), (4, [6, 5, 6, 3], 1, 0),        # effort 9: 11 leaves per channel
    (1, [5, 1], 0, 1), (1, [4, 5], 0, 2)])                                                    # palette: indices, then the colours
def test_searched_tree_reads_back_and_its_walks_end_where_the_table_says(nch, preds, wp_ctx, palette):
    err = api.ErrorInfo()
    arr = (C.c_int32 * len(preds))(*preds)
    assert _lib().jxlhip_selftest_lossless_tree(nch, arr, wp_ctx, palette, C.byref(err)) == 0, err.errorMessage


def _file(w, h, nch, colours):
    buf = (C.c_uint8 * (1 << 20))()
    n = _lib().jxlhip_selftest_lossless_file(w, h, nch, colours, buf, len(buf))
    assert n > 0
    return bytes(buf[:n])


@pytest.mark.parametrize("w,h,nch,colours", [(40, 30, 4, 5), (256, 3, 3, 256), (1, 1, 2, 1), (7, 256, 4, 17)])
def test_palette_file_written_by_the_host_pieces_parses_and_decodes(oracle, w, h, nch, colours):
    data = _file(w, h, nch, colours)
    st, _, msg = api.parse_check(data)
    assert st == "Ok", msg
    y, x = np.mgrid[0:h, 0:w]
    idx = (x + 2 * y) % colours
    want = np.stack([(37 * idx + 91 * c) & 255 for c in range(nch)], axis=-1).astype(np.uint8)
    got = oracle.decode(data).pixels
    assert got.shape == want.shape and (got == want).all()


@pytest.mark.parametrize("w,h,nch", [(1, 1, 1), (33, 9, 2), (256, 2, 3), (20, 70, 4)])
def test_effort9_tree_in_a_file_parses_and_decodes(oracle, w, h, nch):
    """Every sample zero: the weighted predictor and property 15 are then 0 everywhere, so the file needs no predictor state on the
    writing side, and the decoders still walk the channel split and the property-15 search of every sample."""
    data = _file(w, h, nch, 0)
    st, _, msg = api.parse_check(data)
    assert st == "Ok", msg
    got = oracle.decode(data).pixels
    assert got.shape == (h, w, nch) and (got == 0).all()
