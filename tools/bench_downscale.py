"""Times the batch API on 3840 x 2160 lossy frames (distance 1), opaque and RGBA, at full size against the reduced-size decode
(decoder option "downscale" = 8): one image and a batch of 32, the two scales alternating in one process, warm, best of 7 (host clock
around a synchronised decode_batch), with the device time per stage of the last decode of each kind.
`profile` as argv[1]: a few reduced decodes only (an opaque and an RGBA lossy frame, and a lossless RGBA frame for box_reduce_kernel),
for a run under rocprofv3 --kernel-trace --stats; the JSON line then carries the bytes each of the three kernels moves, from the
shapes.  DESIGN.md §4.12 records the numbers.  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth

W, H, BATCH, REPS, SEEDS = 3840, 2160, 32, 7, 2
CELLS = ((W + 7) // 8) * ((H + 7) // 8)

images = [synth(W, H, 11 + s) for s in range(SEEDS)]
files = {"rgba": [O.encode(im, distance=1.0) for im in images], "opaque": [O.encode(np.ascontiguousarray(im[..., :3]), distance=1.0) for im in images]}
dec = api.Decoder(0)


def run(batch, scale):
    """Wall time in ms of one synchronised batch at the given scale, and its stage times."""
    info = api.peek(batch[0])
    outs = run.outs.setdefault((len(batch), info.num_channels), [torch.empty(W * H * info.num_channels, dtype=torch.uint8, device="cuda") for _ in batch])
    assert dec.set_option("downscale", scale) == 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = dec.decode_batch(batch, [o.data_ptr() for o in outs])
    ms = (time.perf_counter() - t0) * 1e3
    assert all(s == 0 for s in st), st
    return ms, dec.stage_times()


run.outs = {}

if sys.argv[1:] == ["profile"]:
    lossless = api.save_image(np.ascontiguousarray(images[0][..., [2, 1, 0, 3]]), lossless=True)
    for _ in range(4):
        for f in (files["opaque"][0], files["rgba"][0], lossless):
            run([f], 8)
    print(json.dumps({"case": "profile: 4K opaque lossy, RGBA lossy, RGBA lossless at 1:8", "cells": CELLS,
                      "lf_output_bytes": {"opaque": CELLS * (12 + 3), "rgba": CELLS * (12 + 1 + 4)},
                      "alpha_reduce_bytes": W * H + CELLS, "box_reduce_bytes": 4 * W * H + 4 * CELLS}), flush=True)
    sys.exit(0)

result = {"case": "3840x2160 lossy, distance 1; decode_batch, synchronised; ms, best of %d, scales alternating" % REPS, "cases": {}}
for kind in ("opaque", "rgba"):
    for n in (1, BATCH):
        batch = [files[kind][i % SEEDS] for i in range(n)]
        for scale in (1, 8):   # warm: workspace, code objects
            run(batch, scale)
        ts, stages = {1: [], 8: []}, {}
        for _ in range(REPS):
            for scale in (1, 8):
                ms, stages[scale] = run(batch, scale)
                ts[scale].append(ms)
        result["cases"]["%s_b%d" % (kind, n)] = {
            "full_ms": round(min(ts[1]), 3), "downscale8_ms": round(min(ts[8]), 3), "all_full": [round(t, 3) for t in ts[1]],
            "all_downscale8": [round(t, 3) for t in ts[8]], "stages_full": {k: round(v, 3) for k, v in stages[1].items()},
            "stages_downscale8": {k: round(v, 3) for k, v in stages[8].items()}}
dec.set_option("downscale", 1)
print(json.dumps(result), flush=True)
