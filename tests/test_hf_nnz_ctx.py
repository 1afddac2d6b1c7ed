"""CPU check of the register form of the HF non-zero-count bucket (NnzBucketCtx in csrc/dev_util.h) that the batched HF token
loop uses in place of a table lookup: all 64 inputs against the table of the format's coefficient context model."""
import ctypes as C

from pdn_jpegxl_amd import api

# context offset of the coefficient tokens for a predicted non-zero count of 0 .. 63 (buckets 0, 1, 2, 3-4, 5-8, 9-12, 13-20, 21-32, 33-63
# in units of 31 contexts, less the unused lowest ones)
TABLE = [0, 0, 31, 62, 62] + [93] * 4 + [123] * 4 + [152] * 8 + [180] * 12 + [206] * 31


def test_nnz_bucket_in_registers_equals_the_table():
    assert len(TABLE) == 64
    L = api.selftest_lib()
    L.jxlhip_selftest_nnz_ctx.restype = C.c_uint32
    L.jxlhip_selftest_nnz_ctx.argtypes = [C.c_uint32]
    got = [L.jxlhip_selftest_nnz_ctx(n) for n in range(64)]
    assert got == TABLE
