"""Times LoadImage on a 3840 x 2160 RGBA lossy frame (distance 1) with synthetic noise (a mid-strength ramp of strengths) and without,
alternating, warm, and prints the device time of the noise stage (the generator and the convolution) of the last noisy decode.
`profile` as argv[1]: a few noisy decodes only, for a run under rocprofv3 --kernel-trace --stats.  DESIGN.md §4.9 records the numbers.
Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import noise_util as NU
import oracle_lib as O
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth

W, H = 3840, 2160
RAMP = list(range(0, 512, 64))

plain = O.encode(synth(W, H, 11), distance=1.0, container=False)
noisy = NU.noisy(plain, RAMP)

if sys.argv[1:] == ["profile"]:
    for _ in range(4):
        api.load_image(noisy)
    sys.exit(0)

for data in (plain, noisy):
    api.load_image(data)
ts = {"plain": [], "noise": []}
stages, stages_plain = {}, {}
for _ in range(7):
    for name, data in (("plain", plain), ("noise", noisy)):
        t0 = time.perf_counter()
        api.load_image(data)
        ts[name].append((time.perf_counter() - t0) * 1e3)
        if name == "noise":
            stages = api.last_load_stage_times()
        else:
            stages_plain = api.last_load_stage_times()
groups = ((W + 255) // 256) * ((H + 255) // 256)
print(json.dumps({"case": "4K RGBA lossy, distance 1", "loadimage_ms_plain": round(min(ts["plain"]), 2), "loadimage_ms_noise": round(min(ts["noise"]), 2),
                  "all_plain": [round(t, 2) for t in ts["plain"]], "all_noise": [round(t, 2) for t in ts["noise"]],
                  "noise_stage_ms": round(stages.get("noise", -1.0), 3), "stages_noise": {k: round(v, 3) for k, v in stages.items()},
                  "stages_plain": {k: round(v, 3) for k, v in stages_plain.items()},
                  "groups": groups, "generator_steps_per_group": 3 * 256 * 16, "plane_bytes": 3 * 4 * W * H}), flush=True)
