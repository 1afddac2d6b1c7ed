"""What fitting the chroma-from-luma maps costs and saves (JxlHipLossyOptions::chroma_from_luma): one 3840 x 2160 RGBA8 frame from synth
through jxlhip_save_pixels_lossy at efforts 7 and 8, and a batch of 32 such frames through jxlhip_encode_batch_lossy at effort 7 (a
batch refuses 8), each with fitting off and on: bytes, PSNR of the product's decode against the source, wall-clock time per image and
the device time of the `front_end` and `tokens + histograms` stages.  One process, warm, the cases alternating, every sample kept; a
case's figure is its best round.

--parent-lib PATH: a build of the parent commit's library.  The off path's front_end time of this build is then compared with the
parent's, the two alternating round by round through jxlhip_save_pixels; they must be level within the spread of the repeats
(exit status 1 otherwise).  Writes profiles/cfl_bench.json and prints the same JSON line (DESIGN.md §4.6 records the numbers)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISTINCT = 4
FRONT, TOKENS = "front_end", "tokens + histograms"


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def stage(times, prefix):
    return round(sum(v for k, v in times.items() if k.startswith(prefix)), 3)


def raw_front_end_ms(L, api, px):
    """One effort-7 save of px through jxlhip_save_pixels of library L; its front_end stage time in ms."""
    h, w, c = px.shape
    desc = api.JxlHipPixels(px.ctypes.data, w, h, w * c, c, 0, 8, api.KNOWN_PROFILE.index("Srgb"))
    io = api.IOCallbacks(api.WriteFn(lambda p, n: api.S_OK), api.SeekFn(lambda p: api.S_OK))
    err = api.ErrorInfo()
    st = L.jxlhip_save_pixels(C.byref(desc), C.byref(api.EncoderOptions(1.0, 7, False)), C.byref(api.EncoderImageMetadata()), C.byref(io),
                              C.byref(err), api.ProgressFn())
    if st != 0:
        sys.exit("jxlhip_save_pixels failed: " + err.errorMessage.decode("ascii", "replace"))
    names, ms = (C.c_char_p * 16)(), (C.c_float * 16)()
    k = L.jxlhip_last_save_stage_times(names, ms, 16)
    return sum(ms[i] for i in range(k) if names[i].decode().startswith(FRONT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from pdn_jpegxl_amd import api
    from pdn_jpegxl_amd.synth import synth
    W, H = args.width, args.height
    host = [synth(W, H, 2 + k) for k in range(DISTINCT)]
    dev = [torch.from_numpy(p).cuda() for p in host]
    torch.cuda.synchronize()
    enc = api.Encoder(0)
    res = {"case": "%dx%d RGBA8 from synth, distance 1; one process, warm, cases alternating, best of %d rounds (effort 8: of %d)"
                   % (W, H, args.rounds, max(2, args.rounds // 2))}

    # ---- one frame
    single = {}
    for effort in (7, 8):
        rounds = args.rounds if effort == 7 else max(2, args.rounds // 2)
        cases = {"off": False, "on": True}
        files = {name: api.save_pixels(host[0], distance=1.0, effort=effort, cfl=cfl) for name, cfl in cases.items()}   # warm
        ts = {name: [] for name in cases}
        front = {name: [] for name in cases}
        tokens = {name: [] for name in cases}
        for _ in range(rounds):
            for name, cfl in cases.items():
                t0 = time.perf_counter()
                api.save_pixels(host[0], distance=1.0, effort=effort, cfl=cfl)
                ts[name].append((time.perf_counter() - t0) * 1e3)
                st = api.last_save_stage_times()
                front[name].append(stage(st, FRONT))
                tokens[name].append(stage(st, TOKENS))
        out = {}
        for name in cases:
            px = api.load_image(files[name]).pixels
            out[name] = {"bytes": len(files[name]), "psnr_db": round(psnr(px[..., :3], host[0][..., :3]), 3), "wall_ms": round(min(ts[name]), 2),
                         "front_end_ms": min(front[name]), "tokens_histograms_ms": min(tokens[name]),
                         "all_wall_ms": [round(t, 2) for t in ts[name]], "all_front_end_ms": front[name]}
        out["bytes_on_over_off"] = round(out["on"]["bytes"] / out["off"]["bytes"], 4)
        out["psnr_on_minus_off_db"] = round(out["on"]["psnr_db"] - out["off"]["psnr_db"], 3)
        single["effort %d" % effort] = out
    res["single"] = single

    # ---- a batch
    n = args.batch
    batches = {name: [api.EncodeItem.from_tensor(dev[k % DISTINCT], distance=1.0, effort=7, cfl=cfl) for k in range(n)]
               for name, cfl in (("on", True), ("off", False))}
    files = {name: enc.encode_batch(items) for name, items in batches.items()}   # warm, the larger workspace first
    ts = {name: [] for name in batches}
    stages = {}
    for _ in range(args.rounds):
        for name, items in batches.items():
            t0 = time.perf_counter()
            enc.encode_batch(items)
            dt = (time.perf_counter() - t0) * 1e3
            ts[name].append(dt)
            if dt <= min(ts[name]):
                stages[name] = {k: round(v, 3) for k, v in enc.stage_times().items()}
    batch = {}
    for name in ("off", "on"):
        shown = min(n, DISTINCT)
        ps = [psnr(api.load_image(files[name][k]).pixels[..., :3], host[k][..., :3]) for k in range(shown)]
        batch[name] = {"bytes": sum(len(f) for f in files[name]), "psnr_db_mean_of_%d" % shown: round(float(np.mean(ps)), 3),
                       "wall_ms_per_image": round(min(ts[name]) / n, 3), "all_wall_ms": [round(t, 2) for t in ts[name]],
                       "front_end_and_tokens_ms": stage(stages[name], "pixels, front end, tokens"), "stages_ms": stages[name]}
    batch["bytes_on_over_off"] = round(batch["on"]["bytes"] / batch["off"]["bytes"], 4)
    batch["equals_single_call"] = files["on"][0] == api.save_pixels(host[0], distance=1.0, effort=7, cfl=True)
    res["batch of %d, effort 7" % n] = batch
    enc.close()

    # ---- the off path against the parent commit's library
    level = True
    if args.parent_lib:
        libs = {"parent": C.CDLL(os.path.abspath(args.parent_lib)), "this": api.lib()}
        for L in libs.values():
            L.jxlhip_save_pixels.restype = C.c_int32
            L.jxlhip_last_save_stage_times.restype = C.c_int32
            raw_front_end_ms(L, api, host[0])   # warm
        fe = {name: [] for name in libs}
        for _ in range(2 * args.rounds):
            for name, L in libs.items():
                fe[name].append(round(raw_front_end_ms(L, api, host[0]), 3))
        med = {name: float(np.median(v)) for name, v in fe.items()}
        spread = max(max(v) - min(v) for v in fe.values())
        level = abs(med["this"] - med["parent"]) <= spread
        res["off path front_end against the parent commit"] = {
            "rounds": 2 * args.rounds, "median_ms": {k: round(v, 3) for k, v in med.items()}, "min_ms": {k: min(v) for k, v in fe.items()},
            "spread_ms": round(spread, 3), "level_within_spread": level, "all_ms": fe}

    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "cfl_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    if not batch["equals_single_call"]:
        sys.exit("a file of the batch differs from the single call's")
    if not level:
        sys.exit("the off path's front_end time differs from the parent's by more than the spread of the repeats")


if __name__ == "__main__":
    main()
