"""Times animation encode (api.Encoder.encode_animation) per frame against encode_batch of the same frames as unrelated full-frame
stills - the path there was before - alternating in one process:
  sprite:  32 frames of 3840 x 2160 RGBA8, a static synthetic background with a 256 x 256 sprite that moves every frame;
  changed: the same size, every sample of every frame differs from its predecessor (the worst case: what the extents pass and the
           assembly cost on top of the batch);
each lossy (distance 1, effort 7) and lossless.  Times are HIP events around the synchronous calls (host work included), best and
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


def run(name, make, lossless, rounds, only_animation):
    frames = make()
    kw = dict(lossless=True) if lossless else dict(distance=1.0, effort=7)
    items = [api.EncodeItem.from_tensor(f, **kw) for f in frames]
    enc = api.Encoder(0)
    t_anim, t_batch, t_ext = [], [], []
    out = {}
    for r in range(rounds + 1):
        ta = timed(lambda: out.__setitem__("anim", enc.encode_animation(items, 1, **kw)))
        ext = enc.stage_times().get(EXTENTS_STAGE, 0.0)
        rects = enc.last_animation_rects
        tb = 0.0 if only_animation else timed(lambda: out.__setitem__("batch", enc.encode_batch(items)))
        if r:
            t_anim.append(ta), t_batch.append(tb), t_ext.append(ext)
    enc.close()
    ext_bytes = 2 * (N - 1) * W * H * 4
    ext_ms = min(t_ext)
    line = {"case": "%s, %dx%d RGBA8, %d frames, %s" % (name, W, H, N, "lossless" if lossless else "lossy d1 e7"),
            "coded_pixels_share": round(sum(r[2] * r[3] for r in rects) / float(N * W * H), 4),
            "animation_file_bytes": len(out["anim"]),
            "animation_ms_per_frame_best": round(min(t_anim) / N, 3), "animation_ms_per_frame_median": round(statistics.median(t_anim) / N, 3),
            "extents_ms": round(ext_ms, 4), "extents_bytes_read": ext_bytes,
            "extents_tb_per_s": round(ext_bytes / (ext_ms * 1e-3) / 1e12, 3) if ext_ms else None,
            "extents_share_of_copy_rate": round(ext_bytes / (ext_ms * 1e-3) / COPY_RATE, 3) if ext_ms else None, "rounds": rounds}
    if not only_animation:
        line.update({"batch_of_full_frames_bytes": sum(len(b) for b in out["batch"]),
                     "batch_of_full_frames_ms_per_frame_best": round(min(t_batch) / N, 3),
                     "batch_of_full_frames_ms_per_frame_median": round(statistics.median(t_batch) / N, 3)})
    return line


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
    makers = {"sprite": frames_sprite, "changed": frames_changed}
    lines = []
    for case in args.cases:
        what, mode = case.split("-")
        lines.append(run(what, makers[what], mode == "lossless", args.rounds, args.only_animation))
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")
