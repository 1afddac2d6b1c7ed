"""CPU checks of the HF token context rules that every loop of hf_decode_kernel calls (HfPosCtx, HfNnzPredict, HfNnzCountBucket in
csrc/dev_util.h), each against the format's definition written out here independently.  Exhaustive over the reachable inputs."""
import ctypes as C

from pdn_jpegxl_amd import api


def _fn(name, nargs):
    f = getattr(api.selftest_lib(), name)
    f.restype = C.c_uint32
    f.argtypes = [C.c_uint32] * nargs
    return f


def test_position_context_equals_the_piecewise_definition():
    pos_ctx = _fn("jxlhip_selftest_hf_pos_ctx", 1)

    def piecewise(ks):
        if ks < 16:
            return ks - 1
        if ks < 32:
            return 15 + ((ks - 16) >> 1)
        return 23 + ((ks - 32) >> 2)

    assert [pos_ctx(ks) for ks in range(1, 64)] == [piecewise(ks) for ks in range(1, 64)]


def test_nonzero_count_context_for_every_edge_and_neighbour_pair():
    predict = _fn("jxlhip_selftest_hf_nnz_predict", 4)
    bucket = _fn("jxlhip_selftest_hf_nnz_bucket", 1)

    def want(bx, by, above, left):
        if bx == 0 and by == 0:
            p = 32
        elif bx == 0:
            p = above
        elif by == 0:
            p = left
        else:
            p = (above + left + 1) // 2
        p = min(p, 64)
        return p if p < 8 else 4 + p // 2

    for bx in (0, 1, 31):
        for by in (0, 1, 31):
            got = [bucket(predict(bx, by, a, l)) for a in range(65) for l in range(65)]
            assert got == [want(bx, by, a, l) for a in range(65) for l in range(65)], (bx, by)
    # the clamp: a prediction above 64 (a corrupt count) lands in the last bucket, 4 + 64 / 2
    assert [bucket(p) for p in (64, 65, 255, 1 << 20)] == [36] * 4
