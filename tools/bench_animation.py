"""Times the animation decode (api.Animation.next) per displayed image against jxlhip_decode_batch of the same frames as single-frame
files, alternating in one process, and prints the compositor's bytes:
  lossless: 4K RGBA Modular, 32 full-canvas kReplace frames (output-type samples, selected);
  lossy:    4K RGBA VarDCT, 32 full-canvas kReplace frames;
  blend:    4K RGBA Modular canvas, 32 frames that are each a 1024 x 768 kBlend crop onto slot 1 and saved to slot 1 (f32 frames);
  blend-cut8: the same file with the option "chunk_frames" = 8, so that slot 1 crosses three cuts (what a cut costs).
Times are HIP events around the synchronous calls (host work included), best and median of `--rounds`; compose_kernel's time is the
"compose" stage of the animation's decoder summed over the chunks of one pass.  The batch path runs no code this feature changed: it is
the yardstick.  One JSON line per case; --out also writes them to a file (profiles/animation_bench.json).

Two further cases time random access and thumbnails on a file the product's own encoder writes - 4K RGBA lossless, 32 frames, a
256 x 256 block moving over a background that changes at every key frame, key_interval 8, so the entry points are 0, 8, 16, 24:
  seek:   seek(j); next(1) against rewind(); next(j + 1), for j = 7, 15, 20 and 31;
  thumbs: rewind(); thumbnails of all 32 images (and of every fourth) against rewind(); next(32) at full size."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import animation_util as AU
import layer_util as LU
import oracle_lib as O
from pdn_jpegxl_amd import api
from pdn_jpegxl_amd.synth import synth

W, H, N = 3840, 2160, 32   # --width / --height / --frames change them (a quick run; the recorded figures are of the defaults)
COPY_RATE = 6.29e12   # float4 copy, bytes per second read + written


def frames_lossless():
    kw = dict(lossless=True, container=False, lossless_tree=1, lossless_predictor=5)
    pics = [O.encode(synth(W, H, 2 + s), **kw) for s in range(4)]   # four pictures in turn: the files are as long as 32 distinct ones
    canvas = O.encode(np.zeros((H, W, 4), np.uint8), animation_frames=2, **kw)
    layers = [LU.Layer(pics[k % 4], crop=False, duration=1) for k in range(N)]
    return "%dx%d RGBA lossless, %d full-canvas kReplace frames" % (W, H, N), canvas, layers, [pics[k % 4] for k in range(N)], 4


def frames_lossy():
    kw = dict(distance=1.0, container=False)
    pics = [O.encode(synth(W, H, 11 + s), **kw) for s in range(4)]
    canvas = O.encode(synth(W, H, 11), animation_frames=2, **kw)
    layers = [LU.Layer(pics[k % 4], crop=False, duration=1) for k in range(N)]
    return "%dx%d RGBA lossy, %d full-canvas kReplace frames" % (W, H, N), canvas, layers, [pics[k % 4] for k in range(N)], 4


def frames_blend():
    kw = dict(lossless=True, container=False, lossless_tree=1, lossless_predictor=5)
    cw, ch = min(1024, W), min(768, H)
    pics = [O.encode(synth(cw, ch, 21 + s), **kw) for s in range(4)]
    canvas = O.encode(np.zeros((H, W, 4), np.uint8), animation_frames=2, **kw)
    blend = [LU.Blending(2, 0, False, 1), LU.Blending(2, 0, False, 1)]
    layers = [LU.Layer(pics[k % 4], x0=(97 * k) % max(1, W - cw), y0=(41 * k) % max(1, H - ch), blending=blend, duration=1, save_ref=1)
              for k in range(N)]
    return "%dx%d RGBA lossless canvas, %d frames of %dx%d kBlend onto slot 1, saved to slot 1" % (W, H, N, cw, ch), canvas, layers, [pics[k % 4] for k in range(N)], 16


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run(case, rounds, plan_only, chunk_frames=0):
    title, canvas, layers, singles, sample_bytes = case()
    if chunk_frames:
        title += ', "chunk_frames" = %d' % chunk_frames
    data = LU.layered(canvas, layers)
    p = AU.plan(data, chunk_frames)
    # the compositor's bytes: every frame read once, N canvases written, live slots stored at a cut and loaded behind it
    frame_px = sum(LU.read_image_header(L.cs).xsize * LU.read_image_header(L.cs).ysize for L in layers)
    read_frames = frame_px * sample_bytes
    written = p.num_displayed * W * H * 4
    cuts = sum(bin(c["live_out"]).count("1") for c in p.chunks) * W * H * 16 * 2
    naive_px = sum(sum(LU.read_image_header(L.cs).xsize * LU.read_image_header(L.cs).ysize for L in layers[:k + 1]) for k in range(N))
    line = {"case": title, "file_bytes": len(data), "displayed": p.num_displayed, "chunks": len(p.chunks),
            "chunk_frames": [c["count"] for c in p.chunks], "live_out": [c["live_out"] for c in p.chunks],
            "frame_scratch_bytes_max": max(f["scratch"] for f in p.frames),
            "compose_bytes_frames_read": read_frames, "compose_bytes_canvases_written": written, "compose_bytes_slots_at_cuts": cuts,
            "naive_compose_bytes_computed_not_run": naive_px * sample_bytes + written}
    if plan_only:
        return line
    import torch
    dec = api.Decoder(0)
    infos = [api.peek(f) for f in singles]
    outs = [torch.empty(i.width * i.height * i.num_channels, dtype=torch.uint8, device="cuda") for i in infos]
    ptrs = [o.data_ptr() for o in outs]
    t_anim, t_batch, t_compose = [], [], []
    with api.Animation(data) as a:
        assert a.set_option("chunk_frames", chunk_frames) == 1
        buf = torch.empty(N * a.info.image_bytes, dtype=torch.uint8, device="cuda")
        n, err = api.C.c_int32(0), api.ErrorInfo()

        def anim():
            a.rewind()
            st = a._L.jxlhip_animation_next(a._h, N, buf.data_ptr(), buf.numel(), api.C.byref(n), api.C.byref(err))
            assert st == 0 and n.value == N, err.errorMessage
        for r in range(rounds + 1):   # the first round warms both (workspaces grow)
            a.decoder_stage_totals(reset=True)
            ta = timed(anim)
            totals, chunks = a.decoder_stage_totals()
            tb = timed(lambda: dec.decode_batch(singles, ptrs))
            if r:
                t_anim.append(ta), t_batch.append(tb), t_compose.append(totals.get("compose", 0.0))
    dec.close()
    comp_ms = min(t_compose)
    comp_bytes = read_frames + written + cuts
    line.update({"animation_ms_per_image_best": round(min(t_anim) / N, 3), "animation_ms_per_image_median": round(statistics.median(t_anim) / N, 3),
                 "batch_of_single_frames_ms_per_image_best": round(min(t_batch) / N, 3),
                 "batch_of_single_frames_ms_per_image_median": round(statistics.median(t_batch) / N, 3),
                 "compose_ms_per_pass": round(comp_ms, 4), "compose_tb_per_s": round(comp_bytes / (comp_ms * 1e-3) / 1e12, 3) if comp_ms else None,
                 "compose_share_of_copy_rate": round(comp_bytes / (comp_ms * 1e-3) / COPY_RATE, 3) if comp_ms else None, "rounds": rounds})
    return line


def keyed_file():
    """The 32-frame file with key frames, and its entry points."""
    import torch
    blocks = [synth(min(256, W), min(256, H), 50 + s) for s in range(4)]
    bgs = [torch.from_numpy(synth(W, H, 31 + s)).cuda() for s in range((N + 7) // 8)]
    frames = []
    for k in range(N):
        f = bgs[k // 8].clone()
        b = torch.from_numpy(blocks[k % 4]).cuda()
        x, y = (97 * k) % max(1, W - b.shape[1]), (41 * k) % max(1, H - b.shape[0])
        f[y:y + b.shape[0], x:x + b.shape[1]] = b
        frames.append(f)
    enc = api.Encoder(0)
    try:
        return enc.encode_animation(frames, 1, key_interval=8, lossless=True)
    finally:
        enc.close()


def run_random_access(mode, rounds):
    import torch
    data = keyed_file()
    line = {"case": "%s: %dx%d RGBA lossless, %d frames from encode_animation(key_interval=8)" % (mode, W, H, N), "file_bytes": len(data), "rounds": rounds}
    with api.Animation(data) as a:
        line["entry_points"] = a.entry_points
        line["codestream_frames"] = a.info.num_codestream_frames
        buf = torch.empty(N * a.info.image_bytes, dtype=torch.uint8, device="cuda")
        n, err = api.C.c_int32(0), api.ErrorInfo()

        def full(count, first=0):
            a.seek(first)
            st = a._L.jxlhip_animation_next(a._h, count, buf.data_ptr(), buf.numel(), api.C.byref(n), api.C.byref(err))
            assert st == 0 and n.value == count, err.errorMessage

        def reduced(step):
            a.rewind()
            st = a._L.jxlhip_animation_next_reduced(a._h, N, step, buf.data_ptr(), buf.numel(), api.C.byref(n), api.C.byref(err))
            assert st == 0 and n.value == (N + step - 1) // step, err.errorMessage

        def best_median(fn):
            fn()   # warms (workspaces grow)
            t = [timed(fn) for _ in range(rounds)]
            return round(min(t), 3), round(statistics.median(t), 3)
        if mode == "seek":
            for j in [j for j in (7, 15, 20, 31) if j < N]:
                a.rewind()   # (each timed seek starts from the front of the file, so it jumps to the entry point)
                line["seek_%d_ms_best_median" % j] = best_median(lambda: (a.rewind(), full(1, j)))
                line["sequential_to_%d_ms_best_median" % j] = best_median(lambda: full(j + 1))
        else:
            line["full_size_next_all_ms_best_median"] = best_median(lambda: full(N))
            a.decoder_stage_totals(reset=True)
            line["thumbnails_all_ms_best_median"] = best_median(lambda: reduced(1))
            totals, chunks = a.decoder_stage_totals()
            line["thumbnails_compose_ms_per_pass"] = round(totals.get("compose", 0.0) / (rounds + 1), 4)
            line["thumbnails_every_4th_ms_best_median"] = best_median(lambda: reduced(4))
            a.decoder_stage_totals(reset=True)
            full(N)
            line["full_size_compose_ms_per_pass"] = round(a.decoder_stage_totals()[0].get("compose", 0.0), 4)
    return line


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", default=["lossless", "lossy", "blend", "blend-cut8"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--frames", type=int, default=N)
    ap.add_argument("--plan-only", action="store_true", help="the files, their chunks and the byte arithmetic, without a GPU")
    args = ap.parse_args()
    W, H, N = args.width, args.height, args.frames
    cases = {"lossless": (frames_lossless, 0), "lossy": (frames_lossy, 0), "blend": (frames_blend, 0), "blend-cut8": (frames_blend, 8)}
    lines = []
    for name in args.cases:
        if name in ("seek", "thumbs"):
            lines.append(run_random_access(name, args.rounds))
        else:
            lines.append(run(cases[name][0], args.rounds, args.plan_only, cases[name][1]))
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")
