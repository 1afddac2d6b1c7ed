"""Times LoadImage on a 3840x2160 RGBA screenshot-like lossless image whose ~10 000 glyphs come from patches of one atlas, against the
same image coded as one plain frame, and prints patch_kernel's bytes.  The patched decode is checked against the image byte for byte
first.  patch_kernel's time comes from a run of its own under rocprofv3 --kernel-trace --stats; DESIGN.md §4.8 records both.  Prints
one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import layer_util as LU
import oracle_lib as O
import patch_util as PU
from pdn_jpegxl_amd import api

W, H = 3840, 2160
GW, GH, STEP, KINDS = 8, 12, (24, 32), 96   # glyph size, grid step, glyph kinds in the atlas


def scene():
    rng = np.random.default_rng(1)
    T = np.full((H, W, 4), 255, np.uint8)
    for k in range(12):   # a few flat panels, as in a screenshot
        x, y = rng.integers(0, W - 600), rng.integers(0, H - 400)
        T[y:y + 400, x:x + 600, :3] = rng.integers(0, 256, 3, dtype=np.uint8)
    glyphs = [np.where(rng.random((GH, GW, 1)) < 0.4, rng.integers(0, 120, (1, 1, 4), dtype=np.uint8), 255).astype(np.uint8) for _ in range(KINDS)]
    atlas = np.zeros((GH, KINDS * GW, 4), np.uint8)
    for g in range(KINDS):
        atlas[:, g * GW:(g + 1) * GW] = glyphs[g]
    coded = T.copy()
    places = [[] for _ in range(KINDS)]
    for y in range(4, H - GH, STEP[1]):
        for x in range(4, W - GW, STEP[0]):
            g = int(rng.integers(0, KINDS))
            T[y:y + GH, x:x + GW] = glyphs[g]
            coded[y:y + GH, x:x + GW] = 0
            places[g].append((x, y))
    refs = [PU.Ref(0, g * GW, 0, GW, GH, [PU.Place(x, y, [(PU.REPLACE, 0, False)] * 2) for x, y in pl]) for g, pl in enumerate(places) if pl]
    return T, coded, atlas, refs


def best(data, reps=5):
    api.load_image(data)
    ts, stages = [], {}
    for _ in range(reps):
        t0 = time.perf_counter()
        api.load_image(data)
        ts.append(time.perf_counter() - t0)
        if ts[-1] == min(ts):
            stages = api.last_load_stage_times()
    return min(ts) * 1e3, stages


def main():
    kw = dict(lossless=True, container=False, lossless_tree=1, lossless_predictor=5)
    T, coded, atlas, refs = scene()
    plain = O.encode(T, **kw)
    patched = LU.layered(plain, [LU.Layer(O.encode(atlas, **kw), frame_type=2), LU.Layer(PU.patched(O.encode(coded, **kw), refs, 1), crop=False, flags=2)])
    got = api.load_image(patched).pixels
    assert (got == T).all(), int((got != T).sum())
    npos = sum(len(r.places) for r in refs)
    # patch_kernel's algorithmic bytes (16 B per f32 RGBA pixel): each tile's box (the union of its positions' rectangles) read, the
    # atlas read once per covered pixel, the covered pixels written
    boxes = {}
    for r in refs:
        for p in r.places:
            for ty in range(p.y // 64, (p.y + GH - 1) // 64 + 1):
                for tx in range(p.x // 64, (p.x + GW - 1) // 64 + 1):
                    b = (max(p.x, tx * 64), max(p.y, ty * 64), min(p.x + GW, tx * 64 + 64), min(p.y + GH, ty * 64 + 64))
                    o = boxes.get((tx, ty), b)
                    boxes[(tx, ty)] = (min(o[0], b[0]), min(o[1], b[1]), max(o[2], b[2]), max(o[3], b[3]))
    covered = npos * GW * GH
    kernel_bytes = 16 * (sum((b[2] - b[0]) * (b[3] - b[1]) for b in boxes.values()) + 2 * covered)
    if len(sys.argv) > 1 and sys.argv[1] == "--profile-only":   # under rocprofv3: a few decodes of the patched file alone
        for _ in range(3):
            api.load_image(patched)
        return
    t_patched, st_patched = best(patched)
    t_plain, _ = best(plain)
    print(json.dumps({"case": "3840x2160 RGBA lossless, %d glyph patches of one %dx%d atlas" % (npos, atlas.shape[1], atlas.shape[0]),
                      "loadimage_ms_patched": round(t_patched, 2), "loadimage_ms_plain": round(t_plain, 2),
                      "stage_ms_patches": round(st_patched.get("patches", -1.0), 4), "tiles_with_patches": len(boxes),
                      "covered_pixels": covered, "patch_kernel_bytes": kernel_bytes, "bytes_patched_file": len(patched), "bytes_plain_file": len(plain)}), flush=True)


if __name__ == "__main__":
    main()
