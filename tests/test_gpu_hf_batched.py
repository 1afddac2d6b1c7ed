"""The batched HF token loop (several sections per wavefront) against the one-section loop and the oracle.

Every case decodes the same files with 64, 8, 4, 2 and 1 lanes between sections: 64 runs the one-section loop (or, for prefix
codes and LZ77, the general loop), the others run the batched loop whose non-zero-count contexts are formed at the block's
descriptor pop.  Outputs must be byte-identical across the mappings and match the oracle.
"""
import re

import numpy as np
import pytest

from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth
from gpu_helpers import gpu_decode

pytestmark = pytest.mark.gpu

STRIDES = (64, 8, 4, 2, 1)


def check_pixels(out, ref):
    assert out.shape == ref.shape
    d = np.abs(out.astype(np.int32) - ref.astype(np.int32))
    assert d.max() <= 1, int(d.max())
    assert (d > 0).mean() <= 2e-3, float((d > 0).mean())
    if out.shape[2] in (2, 4):
        assert (out[..., -1] == ref[..., -1]).all()


def check_mappings(dec, oracle, files):
    refs = [oracle.decode(f).pixels for f in files]
    base = None
    for stride in STRIDES:
        outs = gpu_decode(dec, files, lane_stride=stride)
        for o, r in zip(outs, refs):
            check_pixels(o, r)
        if base is None:
            base = outs
        else:
            for a, b in zip(base, outs):
                assert np.array_equal(a, b), stride


def noise(w, h, seed):
    img = np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3] = 255
    return img


def test_full_blocks_of_non_zeros(gpu_decoder, oracle):
    """Noise at a low distance: (block, channel)s with 63 and more non-zeros, i.e. the top non-zero bucket and the full block."""
    files = [oracle.encode(noise(520, 300, 1), distance=0.1, strategy_mode=1),
             oracle.encode(noise(300, 280, 2), distance=0.3)]
    check_mappings(gpu_decoder, oracle, files)


@pytest.mark.parametrize("strategy", [0, 4, 5, 18, 6, 7, 10, 19])
def test_varblock_sizes(gpu_decoder, oracle, strategy):
    """One varblock size per frame, 8x8 through 64x64 (and rectangles): fills of 1 to 8 columns, predictions across them."""
    img = synth(600, 520, 30 + strategy)
    check_mappings(gpu_decoder, oracle, [oracle.encode(img, strategy_mode=3, fixed_strategy=strategy, distance=0.5)])


def test_mixed_varblocks_in_one_batch(gpu_decoder, oracle):
    files = [oracle.encode(synth(700, 520, 40 + i), strategy_mode=2, seed=i, distance=d) for i, d in enumerate((0.3, 1.0, 3.0))]
    check_mappings(gpu_decoder, oracle, files)


@pytest.mark.parametrize("opts", [dict(lf_contexts=True), dict(num_passes=2), dict(custom_orders=True),
                                  dict(lf_contexts=True, num_passes=2, custom_orders=True)],
                         ids=["lf_contexts", "two_passes", "custom_orders", "all"])
def test_context_variants(gpu_decoder, oracle, opts):
    img = synth(640, 520, 50)
    check_mappings(gpu_decoder, oracle, [oracle.encode(img, strategy_mode=2, seed=5, **opts)])


@pytest.mark.parametrize("opts", [dict(prefix_codes=True), dict(lz77=True)], ids=["prefix", "lz77"])
def test_prefix_and_lz77_streams_keep_the_general_loop(gpu_decoder, oracle, opts):
    img = synth(640, 520, 71)
    img[300:360, :, :] = img[300:301, :, :]
    check_mappings(gpu_decoder, oracle, [oracle.encode(img, **opts)])


def test_flat_frame_of_zero_tokens(gpu_decoder, oracle):
    img = np.full((520, 600, 4), 120, np.uint8)
    img[..., 3] = 255
    check_mappings(gpu_decoder, oracle, [oracle.encode(img)])


def test_sections_of_very_different_sizes(gpu_decoder, oracle):
    """Flat groups beside noisy ones in one frame: lanes of one wavefront finish thousands of tokens apart."""
    img = np.full((768, 1024, 4), 90, np.uint8)
    img[..., 3] = 255
    img[:, 512:] = noise(512, 768, 3)[...]
    img[256:512, :256] = synth(256, 256, 4)
    check_mappings(gpu_decoder, oracle, [oracle.encode(img, distance=0.5), oracle.encode(synth(260, 250, 6))])


def test_corrupt_section_fails_the_same_section(gpu_decoder, oracle):
    """Bytes flipped inside the pass-group sections: every mapping reports a decode error in the same HF section."""
    import torch
    clean = oracle.encode(synth(800, 600, 8))
    info = api.peek(clean)
    out = torch.empty(info.width * info.height * info.num_channels, dtype=torch.uint8, device="cuda")
    tried = 0
    for frac in (0.75, 0.6, 0.85, 0.5):
        data = bytearray(clean)
        at = int(len(data) * frac)
        for k in range(at, at + 16):   # short: one section, so the reported section is not a race between two
            data[k] ^= 0x5A
        sections = []
        for stride in STRIDES:
            gpu_decoder.set_option("lane_stride", stride)
            with pytest.raises(api.FormatError) as e:
                gpu_decoder.decode_batch([bytes(data)], [out.data_ptr()])
            assert e.value.status == "DecodeError"
            m = re.search(r"hf (\d+)", gpu_decoder.last_error)
            sections.append(int(m.group(1)) if m else 0)
        gpu_decoder.set_option("lane_stride", 0)
        assert len(set(sections)) == 1, sections
        if sections[0]:
            tried += 1
    assert tried >= 1   # at least one of the positions hit an HF section
