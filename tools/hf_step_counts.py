#!/usr/bin/env python3
"""Instructions per step of the batched HF token loop: rocprofv3 --pmc counters of hf_decode_kernel divided by the steps its wavefronts took.

Two runs of the SAME command (bench.py --steps 1 --warmup 0 --batch 384 --no-cpu-baseline --sync-steps decodes six batches):
  1. a library built with JXLHIP_EXTRA_CFLAGS=-DJXLHIP_PROFILE_HF, its standard output kept: one "[hfstep]" line per batched wavefront
     (HfProfile::Print in csrc/entropy_kernels.hip) with its steps and the steps on which at least one lane took each path;
  2. the ordinary library under `rocprofv3 --pmc <counters> --output-format csv -d DIR -- python bench.py ...`, counters in a run of
     their own (no tracing beside them); several runs with other counters may be given.

    python tools/hf_step_counts.py --steps-log LOG --pmc DIR_OR_CSV [DIR_OR_CSV ...] [--min-workgroups 32] [--out FILE.json]

Only the batch launches count on both sides: [hfstep] lines and counter rows of launches with at least --min-workgroups workgroups (a
single image is 17).  The counters cover the whole kernel - table staging, the 16-token periods, the epilogue - so "per step" is an upper
bound of the loop body's own count; the periods are 1/16 of the steps."""
import argparse
import collections
import csv
import glob
import json
import os
import re
import sys

WG_THREADS = 512   # hf_decode_kernel's __launch_bounds__
PATHS = ["pops", "nnz", "coef", "tails", "renorms"]


def read_steps(path, min_wg):
    tot = collections.Counter()
    pat = re.compile(r"\[hfstep\] (.*)")
    for line in open(path, errors="replace"):
        m = pat.search(line)
        if not m:
            continue
        f = m.group(1).split()
        rec = {f[i]: int(f[i + 1]) for i in range(0, len(f) - 1, 2)}
        if rec["workgroups"] < min_wg:
            continue
        tot["wavefronts"] += 1
        for k in ["sections", "cycles", "steps"] + PATHS:
            tot[k] += rec[k]
        tot["fill_cols"] += rec["fill_cols"]   # columns of the widest lane at a non-zero count, added up over those steps
        tot["longest_wavefront_steps"] = max(tot["longest_wavefront_steps"], rec["steps"])
    return tot


def read_pmc(paths, min_wg):
    files = []
    for p in paths:
        files += glob.glob(os.path.join(p, "**", "*counter_collection.csv"), recursive=True) if os.path.isdir(p) else [p]
    acc = collections.defaultdict(float)
    launches = collections.Counter()
    for f in files:
        seen = set()
        for row in csv.DictReader(open(f)):
            if "hf_decode_kernel" not in row["Kernel_Name"] or int(row.get("Grid_Size", 0) or 0) < min_wg * WG_THREADS:
                continue
            acc[row["Counter_Name"]] += float(row["Counter_Value"])
            seen.add((row.get("Dispatch_Id"), row["Counter_Name"]))
        for _, name in seen:
            launches[name] += 1
    return dict(acc), dict(launches)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps-log", required=True)
    ap.add_argument("--pmc", nargs="*", default=[])
    ap.add_argument("--min-workgroups", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    st = read_steps(a.steps_log, a.min_workgroups)
    if not st["steps"]:
        sys.exit("no [hfstep] line of a batch launch in %s" % a.steps_log)
    steps = st["steps"]
    res = {"wavefronts": st["wavefronts"], "sections_per_wavefront": round(st["sections"] / st["wavefronts"], 2), "steps": steps,
           "longest_wavefront_steps": st["longest_wavefront_steps"],
           "cycles_per_step_profile_build": round(st["cycles"] / steps, 1),
           "share_of_steps_headed_by": {k: round(st[k] / steps, 4) for k in PATHS},
           "widest_lane_columns_per_nnz_step": round(st["fill_cols"] / max(1, st["nnz"]), 3)}
    counters, launches = read_pmc(a.pmc, a.min_workgroups)
    if counters:
        res["counters"] = {k: int(v) for k, v in sorted(counters.items())}
        res["counter_launches"] = launches
        res["per_step"] = {k: round(v / steps, 2) for k, v in sorted(counters.items())}
        inst = sum(v for k, v in counters.items() if k.startswith("SQ_INSTS_") and k != "SQ_INSTS_VMEM")
        if inst:
            res["instructions_per_step"] = round(inst / steps, 1)
        if "SQ_WAVE_CYCLES" in counters:   # the counter taken to tick once per four shader cycles (the micro-architecture guide's unit for the SQ cycle counters; not measured here)
            res["wave_cycles_per_step"] = round(4 * counters["SQ_WAVE_CYCLES"] / steps, 1)
            if inst:
                res["wave_cycles_per_instruction"] = round(4 * counters["SQ_WAVE_CYCLES"] / inst, 2)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
