"""Times animation encode (api.Encoder.encode_animation) per frame against encode_batch of the same frames as unrelated full-frame
stills - the path there was before - alternating in one process:
  sprite:  32 frames of 3840 x 2160 RGBA8, a static synthetic background with a 256 x 256 sprite that moves every frame;
  changed: the same size, every sample of every frame differs from its predecessor (the worst case: what the extents pass and the
           assembly cost on top of the batch);
  corner:  the sprite case plus a 16 x 16 block that toggles in the opposite corner: two far-apart changes per frame, the case several
           rectangles per frame (max_rects >= 2) are for;
each lossy (distance 1, effort 7) and lossless.  A case name may end in "@M" (sprite-lossy@4): encode_animation runs with max_rects = M
(merge_pixels 4096) and the kernel timed is anim_tiles_kernel; "@1,4" alternates both in one process, round by round, and prints a
line for each.  --frames 2 is the smallest call: one pair.  Times are HIP events around the synchronous calls (host work included), best and
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
MERGE_PIXELS = 4096


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


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run(name, make, lossless, rounds, only_animation, max_rects=(1,)):
    """One line per entry of max_rects; with several they alternate round by round on one encoder."""
    frames = make()
    kw = dict(lossless=True) if lossless else dict(distance=1.0, effort=7)
    items = [api.EncodeItem.from_tensor(f, **kw) for f in frames]
    enc = api.Encoder(0)
    t_anim, t_ext = {m: [] for m in max_rects}, {m: [] for m in max_rects}
    t_batch = []
    out, rects, parts = {}, {}, {}
    for r in range(rounds + 1):
        for m in max_rects:
            ta = timed(lambda: out.__setitem__(m, enc.encode_animation(items, 1, max_rects=m, merge_pixels=MERGE_PIXELS, **kw)))
            ext = enc.stage_times().get(EXTENTS_STAGE if m == 1 else TILES_STAGE, 0.0)
            rects[m], parts[m] = enc.last_animation_rects, enc.last_animation_frame_rects
            if r:
                t_anim[m].append(ta), t_ext[m].append(ext)
        tb = 0.0 if only_animation else timed(lambda: out.__setitem__("batch", enc.encode_batch(items)))
        if r:
            t_batch.append(tb)
    enc.close()
    ext_bytes = 2 * (N - 1) * W * H * 4
    lines = []
    for m in max_rects:
        ext_ms = min(t_ext[m])
        line = {"case": "%s, %dx%d RGBA8, %d frames, %s" % (name, W, H, N, "lossless" if lossless else "lossy d1 e7"),
                "max_rects": m, "codestream_frames": len(parts[m]),
                "coded_pixels_share": round(sum(p[3] * p[4] for p in parts[m]) / float(N * W * H), 4),
                "animation_file_bytes": len(out[m]),
                "animation_ms_per_frame_best": round(min(t_anim[m]) / N, 3), "animation_ms_per_frame_median": round(statistics.median(t_anim[m]) / N, 3),
                "kernel": "anim_extents_kernel" if m == 1 else "anim_tiles_kernel",
                "extents_ms": round(ext_ms, 4), "extents_ms_all_rounds": [round(t, 4) for t in t_ext[m]], "extents_bytes_read": ext_bytes,
                "extents_tb_per_s": round(ext_bytes / (ext_ms * 1e-3) / 1e12, 3) if ext_ms else None,
                "extents_share_of_copy_rate": round(ext_bytes / (ext_ms * 1e-3) / COPY_RATE, 3) if ext_ms else None, "rounds": rounds}
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
    makers = {"sprite": frames_sprite, "changed": frames_changed, "corner": frames_corner}
    lines = []
    for case in args.cases:
        case, _, ms = case.partition("@")
        what, mode = case.split("-")
        for line in run(what, makers[what], mode == "lossless", args.rounds, args.only_animation, tuple(int(m) for m in ms.split(",")) if ms else (1,)):
            lines.append(line)
            print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")
