"""Shared by the chroma-from-luma fit tests (test_cfl_fit_host.py, test_gpu_cfl_fit.py): the two kinds of picture, the oracle's fitted
and zero-map files of a picture (computed once per process, never changed), the maps of a file, error measures."""
import functools

import numpy as np

from pdn_jpegxl_amd import synth as _synth

# (effort of the product, strategy mode of the oracle's encoder with the same transform set): tests/test_gpu_encode.py
EFFORTS = [(3, 1), (5, 4), (7, 0)]
MODES = [1, 4, 0]


@functools.lru_cache(maxsize=None)
def synth_rgb(w, h, seed):
    img = np.ascontiguousarray(_synth.synth(w, h, seed)[:, :, :3])
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def colour_tex(w, h, seed):
    """A texture whose three channels follow ONE pink-noise field with different slopes: chroma follows luma, and not with the
    default factors."""
    t = _synth._pink(np.random.default_rng(seed), h, w, 40.0)
    img = np.stack([128 + t, 60 + 0.15 * t, 200 - 0.8 * t], axis=2)
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    img.setflags(write=False)
    return img


def flat64():
    return np.full((64, 64, 3), 90, np.uint8)


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


_PICTURES = {"synth": synth_rgb, "tex": colour_tex}


@functools.lru_cache(maxsize=None)
def oracle_file(kind, w, h, seed, distance, mode, fitted):
    """The oracle's file of picture (kind, w, h, seed): maps fitted per tile, or all zero."""
    import oracle_lib
    return oracle_lib.encode(_PICTURES[kind](w, h, seed), distance=distance, strategy_mode=mode, side_info=dict(cfl="fitted") if fitted else None)


@functools.lru_cache(maxsize=None)
def oracle_dump(kind, w, h, seed, distance, mode, fitted=True):
    import oracle_lib
    return oracle_lib.decode(oracle_file(kind, w, h, seed, distance, mode, fitted), want_dump=True)


def maps_of(dump):
    """(ytox, ytob) of a decoded file as (tiles down, tiles across) int arrays."""
    wt, ht = (dump.w8 + 7) // 8, (dump.h8 + 7) // 8
    return dump.planes["ytox"].astype(int).reshape(ht, wt), dump.planes["ytob"].astype(int).reshape(ht, wt)


def tiles_that_agree(a, b):
    """Per tile: every cell has the same strategy and raw quant value in both dumps."""
    w8, h8 = a.w8, a.h8
    same = (a.planes["strategy"].reshape(h8, w8) == b.planes["strategy"].reshape(h8, w8)) & \
           (a.planes["raw_quant"].reshape(h8, w8) == b.planes["raw_quant"].reshape(h8, w8))
    wt, ht = (w8 + 7) // 8, (h8 + 7) // 8
    padded = np.ones((ht * 8, wt * 8), bool)
    padded[:h8, :w8] = same
    return padded.reshape(ht, 8, wt, 8).all(axis=(1, 3))
