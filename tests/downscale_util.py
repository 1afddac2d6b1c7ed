"""Helpers for the tests of the reduced-size decode (decoder option "downscale" = 8): a decode that catches writes by
full-size geometry, the float64 reference of the colour rule, and the cell means of the alpha / lossless rules."""
import numpy as np

import noise_util as NU

SENTINEL = 0xA5


def _cdiv(a, b):
    return (a + b - 1) // b


def dtype_of(info):
    """numpy sample type of a file from its `peek` record."""
    if info.bytes_per_sample == 1:
        return np.uint8
    if info.bytes_per_sample == 4:
        return np.float32
    return np.float16 if info.reserved else np.uint16


def decode_reduced_batch(dec, files, factor=8):
    """Decodes the files in one batch with "downscale" = factor.  Every output buffer has the FULL size and is filled with a sentinel,
    so a kernel that addressed the output by full-size geometry lands in owned memory and is caught: every byte behind the reduced
    image must still hold the sentinel.  Returns (statuses, images); the image of a file that failed is None."""
    import torch
    from pdn_jpegxl_amd import api
    infos = [api.peek(f) for f in files]
    outs = [torch.full((i.width * i.height * i.num_channels * i.bytes_per_sample,), SENTINEL, dtype=torch.uint8, device="cuda") for i in infos]
    torch.cuda.synchronize()
    assert dec.set_option("downscale", factor) == 1
    try:
        st = dec.decode_batch(files, [o.data_ptr() for o in outs], raise_on_error=False)
    finally:
        assert dec.set_option("downscale", 1) == 1
    imgs = []
    for s, i, o in zip(st, infos, outs):
        host = o.cpu().numpy()
        rw, rh = api.reduced_size(i.width, i.height, factor)
        nb = rw * rh * i.num_channels * i.bytes_per_sample
        if s != 0:
            assert (host == SENTINEL).all(), "a refused image was written to"
            imgs.append(None)
            continue
        assert (host[nb:] == SENTINEL).all(), "bytes behind the reduced image were written (%d of them)" % int((host[nb:] != SENTINEL).sum())
        imgs.append(host[:nb].view(dtype_of(i)).reshape(rh, rw, i.num_channels).copy())
    return st, imgs


def decode_reduced(dec, data, factor=8):
    st, imgs = decode_reduced_batch(dec, [data], factor)
    assert st == [0], (st, dec.last_error)
    return imgs[0]


def reference_colour(od, dtype=np.uint8):
    """Rule 1 in float64: the oracle's `lf` dump (dequantised, smoothed LF planes X, Y, B of w8 x h8 cells - what the "lf" tap is
    compared with) through XYB -> sRGB -> samples of `dtype`.  Returns (h8, w8, 3)."""
    lf = np.stack([np.asarray(od.planes["lf"][c], np.float64).reshape(od.h8, od.w8) for c in range(3)])
    return NU.to_samples(NU.xyb_to_srgb(lf), dtype)


def _cells(a):
    """(sums over the 8x8 cells in float64 or int64, pixel counts of the cells) of a (h, w[, c]) array; edge cells hold the pixels that exist."""
    a = np.asarray(a)
    sq = a.ndim == 2
    if sq:
        a = a[..., None]
    h, w, c = a.shape
    h8, w8 = _cdiv(h, 8), _cdiv(w, 8)
    wide = np.int64 if a.dtype.kind in "iu" else np.float64
    p = np.zeros((h8 * 8, w8 * 8, c), wide)
    p[:h, :w] = a
    s = p.reshape(h8, 8, w8, 8, c).sum(axis=(1, 3))
    ny = np.minimum(8, h - 8 * np.arange(h8))
    nx = np.minimum(8, w - 8 * np.arange(w8))
    n = (ny[:, None] * nx[None, :])[..., None]
    return (s[..., 0], n[..., 0]) if sq else (s, n)


def box_mean_int(a):
    """(sum + n // 2) // n per 8x8 cell and channel, n = the pixels of the cell that exist; the input's integer type."""
    s, n = _cells(a)
    return ((s + n // 2) // n).astype(np.asarray(a).dtype)


def box_mean_float(a):
    """The mean per 8x8 cell and channel over the pixels that exist, in float64."""
    s, n = _cells(a)
    return s / n
