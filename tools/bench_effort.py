"""Times SaveImage on a 3840 x 2160 RGBA picture at distance 1 at efforts 7, 8 and 9, alternating in one call, warm, best of 7, and
reports per effort the wall time, the stage times (one stage per evaluation of the closed loop), the bytes and the cells over the
loop's target.  argv[1] = directory of another checkout's package (optional, e.g. the parent commit's build): its effort 8 is timed in the
same call, in a child process of its own per round so that both libraries never share a process.  `profile` as argv[1]: two effort-9 saves
only, for a run under rocprofv3 --kernel-trace --stats.  Writes profiles/effort_bench.json and prints the same JSON line.
DESIGN.md §4.10 records the numbers.

`lossless` as argv[1] (argv[2] = the other checkout, optional): the lossless efforts instead, on the same picture and on a 4K picture of
64 colours: bytes, warm SaveImage time (best of 5, efforts alternating) and stage times of efforts 7 / 8 / 9, what the search chose, and
the LoadImage time of each resulting file.  With another checkout, its lossless effort 7 is timed between the rounds (a child process per
round, alternating with this checkout's), which shows the spread of the untouched path.  Writes profiles/lossless_effort.json; DESIGN.md
§4.11 records the numbers."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 3840, 2160
ROUNDS = 7

CHILD = r"""
import sys, time
sys.path.insert(0, sys.argv[1])
import numpy as np
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth
bgra = np.ascontiguousarray(synth(%d, %d, 2)[..., [2, 1, 0, 3]])
api.save_image(bgra, distance=1.0, effort=8)
ts = []
for _ in range(%d):
    t0 = time.perf_counter()
    n = len(api.save_image(bgra, distance=1.0, effort=8))
    ts.append((time.perf_counter() - t0) * 1e3)
print(min(ts), n)
""" % (W, H, ROUNDS)


LL_ROUNDS = 5
LL_CHILD = r"""
import sys, time
sys.path.insert(0, sys.argv[1])
import numpy as np
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth
bgra = np.ascontiguousarray(synth(%d, %d, 2)[..., [2, 1, 0, 3]])
api.save_image(bgra, lossless=True, effort=7)
ts = []
for _ in range(3):
    t0 = time.perf_counter()
    n = len(api.save_image(bgra, lossless=True, effort=7))
    ts.append((time.perf_counter() - t0) * 1e3)
print(min(ts), n)
""" % (W, H)


def few_colours(w, h, ncol):
    """Flat regions and thin lines of ncol colours: the kind of picture a palette is for."""
    import numpy as np
    rng = np.random.default_rng(64)
    cols = rng.integers(0, 256, (ncol, 4), dtype=np.uint8)
    cols[:, 3] = 255
    yy, xx = np.mgrid[0:h, 0:w]
    idx = (xx // 37 + yy // 23 + (xx * yy) // 70001 + ((xx + yy) % 53 == 0) * 7) % ncol
    return np.ascontiguousarray(cols[idx][..., [2, 1, 0, 3]])


def lossless_main(other_dir):
    sys.path.insert(0, ROOT)
    import numpy as np
    from pdn_jpegxl_amd import api
    from pdn_jpegxl_amd.synth import synth
    pictures = {"synth(3840,2160,2) RGBA": np.ascontiguousarray(synth(W, H, 2)[..., [2, 1, 0, 3]]), "64 colours 3840x2160": few_colours(W, H, 64)}
    efforts = (7, 8, 9)
    res = {"case": "lossless SaveImage, warm, best of %d, efforts alternating; LoadImage of each file, warm, best of 3" % LL_ROUNDS, "pictures": {}}
    other_ms = []
    for name, bgra in pictures.items():
        for e in efforts:
            api.save_image(bgra, lossless=True, effort=e)
        ts = {e: [] for e in efforts}
        best, files = {}, {}
        for _ in range(LL_ROUNDS):
            if other_dir and name.startswith("synth"):
                out = subprocess.run([sys.executable, "-c", LL_CHILD, other_dir], stdout=subprocess.PIPE, check=True, timeout=600).stdout.split()
                other_ms.append(round(float(out[0]), 2))
                res["other_checkout_effort_7_bytes"] = int(out[1])
            for e in efforts:
                t0 = time.perf_counter()
                data = api.save_image(bgra, lossless=True, effort=e)
                dt = (time.perf_counter() - t0) * 1e3
                ts[e].append(dt)
                if dt <= min(ts[e]):
                    files[e] = data
                    best[e] = {"ms": round(dt, 2), "bytes": len(data), "info": api.last_save_lossless_info(),
                               "stages_ms": {k: round(v, 3) for k, v in api.last_save_stage_times().items()} if e >= 8 else {}}
        for e in efforts:
            api.load_image(files[e])
            lt = []
            for _ in range(3):
                t0 = time.perf_counter()
                api.load_image(files[e])
                lt.append((time.perf_counter() - t0) * 1e3)
            best[e]["load_ms"] = round(min(lt), 2)
        res["pictures"][name] = {"efforts": {str(e): best[e] for e in efforts}, "all_save_ms": {str(e): [round(t, 2) for t in ts[e]] for e in efforts}}
    if other_ms:
        res["other_checkout_effort_7_ms"] = other_ms
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "lossless_effort.json"), "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


def main():
    if sys.argv[1:2] == ["lossless"]:
        return lossless_main(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.path.insert(0, ROOT)
    import numpy as np
    from pdn_jpegxl_amd import api
    from pdn_jpegxl_amd.synth import synth
    bgra = np.ascontiguousarray(synth(W, H, 2)[..., [2, 1, 0, 3]])
    if sys.argv[1:] == ["profile"]:
        for _ in range(2):
            api.save_image(bgra, distance=1.0, effort=9)
        return
    other = None
    if len(sys.argv) > 1:   # before this process touches the GPU for long: the other checkout's effort 8, same input, same protocol
        out = subprocess.run([sys.executable, "-c", CHILD, sys.argv[1]], stdout=subprocess.PIPE, check=True, timeout=600).stdout.split()
        other = {"ms": round(float(out[0]), 2), "bytes": int(out[1])}
    efforts = (7, 8, 9)
    for e in efforts:
        api.save_image(bgra, distance=1.0, effort=e)
    ts = {e: [] for e in efforts}
    best = {}
    for _ in range(ROUNDS):
        for e in efforts:
            t0 = time.perf_counter()
            data = api.save_image(bgra, distance=1.0, effort=e)
            dt = (time.perf_counter() - t0) * 1e3
            ts[e].append(dt)
            if dt <= min(ts[e]):
                f = api.last_save_distances()
                best[e] = {"ms": round(dt, 2), "bytes": len(data), "stages_ms": {k: round(v, 3) for k, v in api.last_save_stage_times().items()},
                           "evaluations": f["evaluations"], "target": f["target"], "cells": int(f["cells"].size),
                           "cells_over_target_first": f["cells_over_target_first"], "cells_over_target_emitted": f["cells_over_target_emitted"]}
    res = {"case": "3840x2160 RGBA, distance 1, SaveImage warm, best of %d, efforts alternating" % ROUNDS,
           "efforts": {str(e): best[e] for e in efforts}, "all_ms": {str(e): [round(t, 2) for t in ts[e]] for e in efforts},
           "ratio_to_effort_7": {str(e): round(best[e]["ms"] / best[7]["ms"], 2) for e in (8, 9)}}
    if other:
        res["other_checkout_effort_8"] = other
        res["effort_8_ratio_to_other_checkout"] = round(best[8]["ms"] / other["ms"], 2)
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "effort_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
