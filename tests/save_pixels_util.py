"""Helpers of the jxlhip_save_pixels tests (test_save_pixels.py, test_gpu_save_pixels.py): inputs of every sample type, the colour
options of the oracle's encoder that match the host's named profiles, error measures."""
import functools

import numpy as np

from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth, synth16

# KnownColorProfile name -> `colour` option of the oracle's encoder (oracle/jxo_enc.cc: EncodeJxl); the gray profiles are the same
# options with 1 or 2 channels
ORACLE_COLOUR = {"Srgb": 0, "LinearSrgb": 5, "LinearGray": 5, "GraySrgbTRC": 0, "DisplayP3": 1, "Rec709": 2, "Rec2020Linear": 3,
                 "Rec2020PQ": 4}
GRAY_PROFILES = ("LinearGray", "GraySrgbTRC")


def bgra_of(rgba):
    return np.ascontiguousarray(rgba[..., [2, 1, 0, 3]])


def channels(rgba, nch):
    """Gray | Gray,A | R,G,B | R,G,B,A of an RGBA array (gray: the green channel)."""
    if nch == 1:
        return np.ascontiguousarray(rgba[..., 1:2])
    if nch == 2:
        return np.ascontiguousarray(rgba[..., [1, 3]])
    return np.ascontiguousarray(rgba[..., :nch])


def bgra_view(px):
    """The BGRA8 surface SaveImage would be given for the uint8 pixels px (h, w, 1..4): gray replicated, a missing alpha opaque."""
    h, w, c = px.shape
    out = np.empty((h, w, 4), np.uint8)
    if c >= 3:
        out[..., 0], out[..., 1], out[..., 2] = px[..., 2], px[..., 1], px[..., 0]
    else:
        out[..., 0] = out[..., 1] = out[..., 2] = px[..., 0]
    out[..., 3] = px[..., c - 1] if c in (2, 4) else 255
    return out


@functools.lru_cache(maxsize=None)
def _u16(w, h, seed, bits):
    img = synth16(w, h, seed, bits)
    img.setflags(write=False)
    return img


def u16_image(w, h, seed, bits, nch=4):
    """uint16 samples in the low `bits` bits, soft alpha mask."""
    return channels(_u16(w, h, seed, bits), nch)


@functools.lru_cache(maxsize=None)
def _f32(w, h, seed):
    img = synth(w, h, seed).astype(np.float32) / 255.0
    img.setflags(write=False)
    return img


def float_image(w, h, seed, dtype, nch=4, gain=1.0):
    """Float samples on the nominal [0, 1] scale (gain > 1: colour samples above 1; alpha stays inside [0, 1])."""
    img = _f32(w, h, seed).copy()
    img[..., :3] *= gain
    return channels(img, nch).astype(dtype)


def nominal(px, bits=None):
    """Samples on the nominal [0, 1] scale as float64."""
    if px.dtype.kind == "u":
        return px.astype(np.float64) / float((1 << (bits or 8 * px.dtype.itemsize)) - 1)
    return px.astype(np.float64)


def psnr_nominal(a, b):
    mse = np.mean((a - b) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(1.0 / mse)


def save_pixels_raw(desc, opt=None, md=None, with_write=True):
    """jxlhip_save_pixels driven directly: returns (status name, message, number of Write calls)."""
    import ctypes as C
    L = api.lib()
    calls = [0]

    def write(p, n):
        calls[0] += 1
        return api.S_OK

    io = api.IOCallbacks(api.WriteFn(write) if with_write else api.WriteFn(), api.SeekFn(lambda p: api.S_OK))
    err = api.ErrorInfo()
    opt = opt or api.EncoderOptions(1.0, 7, False)
    md = md or api.EncoderImageMetadata()
    st = L.jxlhip_save_pixels(C.byref(desc) if desc is not None else None, C.byref(opt), C.byref(md), C.byref(io), C.byref(err), api.ProgressFn())
    return api.ENCODER_STATUS[st], err.errorMessage.decode("ascii", "replace"), calls[0]
