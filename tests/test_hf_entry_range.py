"""The range rule of the HF token loops (HfEntryFits in csrc/dev_util.h, the check of HfTakeCoeff and HfTakeToken behind kErrRange): a
non-zero coefficient is stored as the int16 half of an entry, so the token values 1 .. 65535 (coefficients -32768 .. 32767) pass and
every larger one is refused.  No writer of this project produces a stream with a wider coefficient (both clamp to +-32767), so the
rule is checked here, on the host, through the function the kernels call."""
import ctypes as C

from pdn_jpegxl_amd import api


def test_entry_range_is_int16():
    L = api.selftest_lib()
    L.jxlhip_selftest_hf_entry_fits.restype = C.c_int32
    L.jxlhip_selftest_hf_entry_fits.argtypes = [C.c_uint32]
    L.jxlhip_selftest_unpack_signed.restype = C.c_int32
    L.jxlhip_selftest_unpack_signed.argtypes = [C.c_uint32]
    fits = L.jxlhip_selftest_hf_entry_fits
    assert L.jxlhip_selftest_unpack_signed(65534) == 32767 and L.jxlhip_selftest_unpack_signed(65535) == -32768
    assert L.jxlhip_selftest_unpack_signed(65536) == 32768 and L.jxlhip_selftest_unpack_signed(65537) == -32769
    assert all(fits(u) == 1 for u in range(0, 65536))
    for u in [65536, 65537, 65538, 1 << 17, (1 << 17) + 1, 1 << 20, (1 << 31) - 1, 1 << 31, (1 << 32) - 2, (1 << 32) - 1]:
        assert fits(u) == 0, u
    # a value that only differs from an int16 above bit 15 must not pass as its low half
    for v16 in (0, 1, -1, 32767, -32768):
        for k in (1, 2, 5, 15):
            v = v16 + (k << 16)
            u = 2 * v if v >= 0 else -2 * v - 1
            assert L.jxlhip_selftest_unpack_signed(u) == v and fits(u) == 0, v
