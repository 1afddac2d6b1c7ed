"""Times animation encode (api.Encoder.encode_animation) per frame against encode_batch of the same frames as unrelated full-frame
stills - the path there was before - alternating in one process:
  sprite:  32 frames of 3840 x 2160 RGBA8, a static synthetic background with a 256 x 256 sprite that moves every frame;
  changed: the same size, every sample of every frame differs from its predecessor (the worst case: what the extents pass and the
           assembly cost on top of the batch);
  corner:  the sprite case plus a 16 x 16 block that toggles in the opposite corner: two far-apart changes per frame, the case several
           rectangles per frame (max_rects >= 2) are for;
each lossy (distance 1, effort 7) and lossless.  A case name may end in "@M" (sprite-lossy@4): encode_animation runs with max_rects = M
(merge_pixels 4096) and the kernel timed is anim_tiles_kernel; "@1,4" alternates both in one process, round by round, and prints a
line for each.  The "noise" cases (noise-lossy@0,4, noise-lossless@0,4) are the sprite stack plus uniform noise of +-2 on every sample,
new for every frame - what a sensor delivers; there the suffix lists TOLERANCES (encode_animation's tolerance; 0: the bits decide and every
frame is written whole), which alternate round by round with max_rects = 4: the stage timed is the one-launch anim_tiles_kernel at
tolerance 0 and, with a tolerance, the whole per-frame loop against the reference canvas (anim_tiles_tol_kernel, the download of the
table, the synchronise, the host's rule, anim_apply_rects_kernel - HIP events around all of it).  --frames 2 is the smallest call: one pair.  Times are HIP events around the synchronous calls (host work included), best and
median of `--rounds` after one warm-up round (workspaces grow in it).  The extents kernel's own time is its stage of the encoder's
stage times (HIP events around the launch); its bytes are the two frames of every pair, read once.  One JSON line per case; --out
also writes them to a file.  --only-animation runs nothing else (for a kernel trace of a short run)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth

W, H, N = 3840, 2160, 32
COPY_RATE = 6.29e12   # float4 copy, bytes per second read + written
EXTENTS_STAGE = "change extents of every pair of frames (one launch)"
TILES_STAGE = "change tiles of every pair of frames (one launch)"
TOLERANCE_STAGE = "change tiles against the reference canvas (a launch per frame)"
MERGE_PIXELS = 4096
NOISE, NOISE_MAX_RECTS = 2, 4


def frames_sprite():
    import torch
    bg = torch.from_numpy(synth(W, H, 41)).cuda()
    sw, sh = min(256, W), min(256, H)
    sprite = torch.from_numpy(synth(sw, sh, 42)).cuda()
    out = []
    for k in range(N):
        f = bg.clone()
        x, y = (131 * k) % max(1, W - sw), (89 * k) % max(1, H - sh)
        f[y:y + sh, x:x + sw] = sprite
        out.append(f)
    return out


def frames_corner():
    out = frames_sprite()
    x, y = W - 24, H - 24                        # the sprite starts at (0, 0) and wanders: this corner is the far one
    for k, f in enumerate(out):
        if k % 2 and x >= 0 and y >= 0:
            f[y:y + 16, x:x + 16] ^= 255
    return out


def frames_changed():
    import torch
    bg = torch.from_numpy(synth(W, H, 41)).cuda()
    return [bg + (37 * k) % 256 for k in range(N)]   # uint8 wraps: every sample differs from its predecessor's by 37


def frames_noise():
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    out = []
    for f in frames_sprite():
        n = torch.randint(-NOISE, NOISE + 1, f.shape, generator=g, device="cuda", dtype=torch.int16)
        out.append((f.to(torch.int16) + n).clamp_(0, 255).to(torch.uint8))   # (clamping keeps two frames within 2 * NOISE of each other)
    return out


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run(name, make, lossless, rounds, only_animation, max_rects=(1,), tolerances=None):
    """One line per entry of max_rects - or, where `tolerances` is given, per tolerance at max_rects = NOISE_MAX_RECTS; with several
    they alternate round by round on one encoder."""
    frames = make()
    kw = dict(lossless=True) if lossless else dict(distance=1.0, effort=7)
    items = [api.EncodeItem.from_tensor(f, **kw) for f in frames]
    enc = api.Encoder(0)
    variants = [(NOISE_MAX_RECTS, float(t)) for t in tolerances] if tolerances else [(m, 0.0) for m in max_rects]
    t_anim, t_ext = {v: [] for v in variants}, {v: [] for v in variants}
    t_batch = []
    out, rects, parts = {}, {}, {}
    stage_of = lambda m, tol: TOLERANCE_STAGE if tol > 0 else (EXTENTS_STAGE if m == 1 else TILES_STAGE)
    for r in range(rounds + 1):
        for v in variants:
            m, tol = v
            ta = timed(lambda: out.__setitem__(v, enc.encode_animation(items, 1, max_rects=m, merge_pixels=MERGE_PIXELS, tolerance=tol, **kw)))
            ext = enc.stage_times().get(stage_of(m, tol), 0.0)
            rects[v], parts[v] = enc.last_animation_rects, enc.last_animation_frame_rects
            if r:
                t_anim[v].append(ta), t_ext[v].append(ext)
        tb = 0.0 if only_animation else timed(lambda: out.__setitem__("batch", enc.encode_batch(items)))
        if r:
            t_batch.append(tb)
    enc.close()
    ext_bytes = 2 * (N - 1) * W * H * 4
    lines = []
    for v in variants:
        m, tol = v
        ext_ms = min(t_ext[v])
        line = {"case": "%s, %dx%d RGBA8, %d frames, %s" % (name, W, H, N, "lossless" if lossless else "lossy d1 e7"),
                "max_rects": m, "codestream_frames": len(parts[v]),
                "coded_pixels_share": round(sum(p[3] * p[4] for p in parts[v]) / float(N * W * H), 4),
                "animation_file_bytes": len(out[v]),
                "animation_ms_per_frame_best": round(min(t_anim[v]) / N, 3), "animation_ms_per_frame_median": round(statistics.median(t_anim[v]) / N, 3),
                "kernel": "anim_tiles_tol_kernel + anim_apply_rects_kernel, a round trip per frame" if tol > 0 else ("anim_extents_kernel" if m == 1 else "anim_tiles_kernel"),
                "extents_ms": round(ext_ms, 4), "extents_ms_all_rounds": [round(t, 4) for t in t_ext[v]], "extents_bytes_read": ext_bytes,
                "extents_tb_per_s": round(ext_bytes / (ext_ms * 1e-3) / 1e12, 3) if ext_ms else None,
                "extents_share_of_copy_rate": round(ext_bytes / (ext_ms * 1e-3) / COPY_RATE, 3) if ext_ms else None, "rounds": rounds}
        if tolerances:
            line.update({"tolerance": tol, "noise": NOISE, "coded_pixels_per_frame": round(sum(p[3] * p[4] for p in parts[v]) / float(N), 1),
                         "extents_ms_per_frame": round(ext_ms / max(1, N - 1), 4)})
        if not only_animation:
            line.update({"batch_of_full_frames_bytes": sum(len(b) for b in out["batch"]),
                         "batch_of_full_frames_ms_per_frame_best": round(min(t_batch) / N, 3),
                         "batch_of_full_frames_ms_per_frame_median": round(statistics.median(t_batch) / N, 3)})
        lines.append(line)
    return lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", default=["sprite-lossy", "sprite-lossless", "changed-lossy", "changed-lossless"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--frames", type=int, default=N)
    ap.add_argument("--only-animation", action="store_true")
    args = ap.parse_args()
    W, H, N = args.width, args.height, args.frames
    makers = {"sprite": frames_sprite, "changed": frames_changed, "corner": frames_corner, "noise": frames_noise}
    lines = []
    for case in args.cases:
        case, _, ms = case.partition("@")
        what, mode = case.split("-")
        if what == "noise":
            suffix = dict(tolerances=tuple(float(t) for t in (ms or "0,4").split(",")))
        else:
            suffix = dict(max_rects=tuple(int(m) for m in ms.split(",")) if ms else (1,))
        for line in run(what, makers[what], mode == "lossless", args.rounds, args.only_animation, **suffix):
            lines.append(line)
            print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")
