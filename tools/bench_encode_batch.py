"""Times jxlhip_encode_batch against a loop of jxlhip_save_pixels on 3840 x 2160 RGBA8 frames (distance 1, effort 7): the batch with
n = 1, 8 and 32 images resident in HBM, the loop of 32 calls on the same pixels in host memory, and a lossless batch of 32.  One
process, warm, the cases alternating, 7 rounds, every sample kept; the figure of a case is its best round divided by its images.
The files of the batch are compared with the loop's (they must be equal).  Writes profiles/encode_batch_bench.json and prints the same
JSON line; exits non-zero when the batch of 32 is not faster per image than the loop by more than the spread of the loop's samples
(DESIGN.md §4.6 records the numbers)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 3840, 2160
ROUNDS = 7
DISTINCT = 4   # pictures the batch cycles through (host memory for the loop's copies, device memory for the batch's)


def main():
    sys.path.insert(0, ROOT)
    import torch
    from pdn_jpegxl_amd import api
    from pdn_jpegxl_amd.synth import synth
    host = [synth(W, H, 2 + k) for k in range(DISTINCT)]
    dev = [torch.from_numpy(p).cuda() for p in host]
    torch.cuda.synchronize()
    enc = api.Encoder(0)

    def items(n, lossless=False):
        return [api.EncodeItem.from_tensor(dev[k % DISTINCT], distance=1.0, effort=7, lossless=lossless) for k in range(n)]

    def loop(n):
        return [api.save_pixels(host[k % DISTINCT], distance=1.0, effort=7) for k in range(n)]

    batches = {n: items(n) for n in (1, 8, 32)}
    ll32 = items(32, lossless=True)
    cases = {
        "encode_batch n=1": (1, lambda: enc.encode_batch(batches[1])),
        "encode_batch n=8": (8, lambda: enc.encode_batch(batches[8])),
        "encode_batch n=32": (32, lambda: enc.encode_batch(batches[32])),
        "loop of 32 save_pixels": (32, lambda: loop(32)),
        "encode_batch n=32 lossless": (32, lambda: enc.encode_batch(ll32)),
    }
    # warm: the largest batch first, so that the workspace is allocated once
    files = {name: cases[name][1]() for name in ("encode_batch n=32", "encode_batch n=32 lossless", "encode_batch n=8", "encode_batch n=1",
                                                 "loop of 32 save_pixels")}
    identical = files["encode_batch n=32"] == files["loop of 32 save_pixels"]
    ll_identical = files["encode_batch n=32 lossless"][:DISTINCT] == [api.save_pixels(p, lossless=True, effort=7) for p in host]
    ts = {name: [] for name in cases}
    stages = {}
    for _ in range(ROUNDS):
        for name, (n, fn) in cases.items():
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            ts[name].append(dt)
            if name.startswith("encode_batch n=32") and dt <= min(ts[name]):
                stages[name] = {k: round(v, 3) for k, v in enc.stage_times().items()}
    per_image = {name: round(min(ts[name]) / cases[name][0], 3) for name in cases}
    loop_ms = [t / 32 for t in ts["loop of 32 save_pixels"]]
    spread = max(loop_ms) - min(loop_ms)
    batch32, loop32 = per_image["encode_batch n=32"], per_image["loop of 32 save_pixels"]
    ok = batch32 < loop32 - spread
    res = {"case": "3840x2160 RGBA8 from synth, distance 1, effort 7; pixels in HBM (batch) / host memory (loop); one process, warm, "
                   "cases alternating, best of %d" % ROUNDS,
           "bytes_equal_loop": identical, "lossless_bytes_equal_save_pixels": ll_identical,
           "per_image_ms": per_image, "loop_per_image_spread_ms": round(spread, 3),
           "batch32_faster_than_loop_by_more_than_spread": ok,
           "stages_ms_n32": stages.get("encode_batch n=32", {}), "stages_ms_n32_lossless": stages.get("encode_batch n=32 lossless", {}),
           "all_ms": {k: [round(t, 2) for t in v] for k, v in ts.items()},
           "file_bytes_n32": sum(len(f) for f in files["encode_batch n=32"])}
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "encode_batch_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    enc.close()
    if not identical or not ll_identical:
        sys.exit("a file of the batch differs from save_pixels'")
    if not ok:
        sys.exit("encode_batch at n = 32 is not faster per image than the loop by more than the loop's spread")


if __name__ == "__main__":
    main()
