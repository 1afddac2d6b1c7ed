"""Times LoadImage on 4K layered files against one of their frames alone as a single-frame file, and prints the compositor's bytes:
  lossless: RGBA Modular, three full-canvas layers + one cropped kBlend layer (f32 frames, blended);
  lossy:    RGBA VarDCT, three kReplace layers, two of them cropped (output-type frames, selected).
compose_kernel's time comes from a run of its own under rocprofv3 --kernel-trace --stats, one case per run (argv[1]); DESIGN.md §4.7
records both.  Prints one JSON line per case."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import layer_util as LU
import oracle_lib as O
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth

W, H = 3840, 2160


def best(data, reps=5):
    api.load_image(data)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        api.load_image(data)
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3


def lossless():
    kw = dict(lossless=True, container=False, lossless_tree=1, lossless_predictor=5)
    full = [synth(W, H, s) for s in (2, 3, 4)]
    top = synth(1024, 768, 5)
    canvas = O.encode(full[0], **kw)
    blend = [LU.Blending(2, 0, False, 0), LU.Blending(2, 0, False, 0)]
    data = LU.layered(canvas, [LU.Layer(O.encode(p, **kw), crop=False) for p in full] + [LU.Layer(O.encode(top, **kw), x0=1400, y0=700, blending=blend)])
    # f32 frames: every covering frame read once (16 B per pixel), the canvas written once (4 B per pixel)
    nbytes = (3 * W * H + top.shape[0] * top.shape[1]) * 16 + W * H * 4
    return "4K RGBA lossless, 3 full layers + 1 cropped kBlend layer", data, canvas, nbytes


def lossy():
    kw = dict(distance=1.0, container=False)
    sizes = [(W, H, None), (2000, 1200, (500, 300)), (1500, 1000, (2600, 1400))]
    files = [O.encode(synth(w, h, 11 + k), **kw) for k, (w, h, _) in enumerate(sizes)]
    data = LU.layered(files[0], [LU.Layer(cs, crop=pos is not None, x0=pos[0] if pos else 0, y0=pos[1] if pos else 0)
                                 for cs, (_, _, pos) in zip(files, sizes)])
    # output-type (u8 RGBA) frames: 4 B per covering pixel read, 4 B per canvas pixel written
    nbytes = sum(w * h for w, h, _ in sizes) * 4 + W * H * 4
    return "4K RGBA lossy, 3 kReplace layers (2 cropped)", data, files[0], nbytes


cases = {"lossless": lossless, "lossy": lossy}
for name in (sys.argv[1:] or list(cases)):
    title, data, single, nbytes = cases[name]()
    print(json.dumps({"case": title, "loadimage_ms_layered": round(best(data), 2), "loadimage_ms_single_frame": round(best(single), 2),
                      "compose_bytes": nbytes, "bytes": len(data)}), flush=True)
