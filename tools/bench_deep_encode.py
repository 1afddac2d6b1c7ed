"""Times jxlhip_save_pixels on one 3840 x 2160 RGBA frame: 16-bit integers lossy, binary32 lossy, 16-bit integers lossless, and
8-bit integers lossy through the same entry - which doubles as the identity check: its bytes must be SaveImage's for the BGRA view of
the same pixels.  Wall time of the call and the stage times of jxlhip_last_save_stage_times, warm, best of 7, the cases alternating.
Writes profiles/deep_encode_bench.json and prints the same JSON line.  DESIGN.md §4.6 records the numbers."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 3840, 2160
ROUNDS = 7


def main():
    sys.path.insert(0, ROOT)
    import numpy as np
    from pdn_jpegxl_amd import api
    from pdn_jpegxl_amd.synth import synth, synth16
    u8 = synth(W, H, 2)
    u16 = synth16(W, H, 2)
    f32 = (u16.astype(np.float32) / 65535.0).astype(np.float32)
    bgra = np.ascontiguousarray(u8[..., [2, 1, 0, 3]])
    cases = {
        "u16 lossy": lambda: api.save_pixels(u16, distance=1.0, effort=7),
        "f32 lossy": lambda: api.save_pixels(f32, distance=1.0, effort=7),
        "u16 lossless": lambda: api.save_pixels(u16, lossless=True, effort=7),
        "u8 lossy (new entry)": lambda: api.save_pixels(u8, distance=1.0, effort=7),
        "u8 lossy (SaveImage)": lambda: api.save_image(bgra, distance=1.0, effort=7),
    }
    files = {name: fn() for name, fn in cases.items()}   # warm
    identical = files["u8 lossy (new entry)"] == files["u8 lossy (SaveImage)"]
    ts = {name: [] for name in cases}
    best = {}
    for _ in range(ROUNDS):
        for name, fn in cases.items():
            t0 = time.perf_counter()
            data = fn()
            dt = (time.perf_counter() - t0) * 1e3
            ts[name].append(dt)
            if dt <= min(ts[name]):
                lossy = "lossless" not in name
                best[name] = {"ms": round(dt, 2), "bytes": len(data), "MP_per_s": round(W * H / dt / 1e3, 1),
                              "stages_ms": {k: round(v, 3) for k, v in api.last_save_stage_times().items()} if lossy else {}}
    res = {"case": "3840x2160 RGBA through jxlhip_save_pixels, effort 7, distance 1 (lossy), warm, best of %d, cases alternating" % ROUNDS,
           "u8_bytes_equal_save_image": identical, "cases": best, "all_ms": {k: [round(t, 2) for t in v] for k, v in ts.items()}}
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "deep_encode_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    if not identical:
        sys.exit("the 8-bit file of jxlhip_save_pixels differs from SaveImage's")


if __name__ == "__main__":
    main()
