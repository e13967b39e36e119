"""Several tiles per query: today's method against one ground encoding per query (encode_ground + localize_region).

    python tools/time_region.py [--out profiles/r06_time_region.json] [--iters 40] [--warmup 3]
    python tools/time_region.py --trace <rocprofv3 kernel_trace.csv> [--out ...]    # add per-kernel times to the JSON

Synthetic weights (weights.generate_state_dict) and inputs (weights.generate_inputs).  Two paths per workload, both against ONE
aerial cache encoded beforehand (encode_aerial is shared and not timed):
  A: localize_cached(grd.repeat_interleave(n), sat_cache, tile_index=flat tiles)    (one ground encoding per (query, tile) pair)
  B: encode_ground(grd) + localize_region(ground_cache, sat_cache, tiles)            (one ground encoding per query)
Workloads: VIGOR-ori-prior (ori_noise 180, circular padding) with 32 queries x 4 tiles from a pool of 32, VIGOR-ori-prior with 1 query
x 2 tiles and Oxford with 1 query x 4 tiles.  One handle per model with the default micro-batch of 32: the 128 pairs run as four
batch-32 plans.  Every case is warmed up first (plans, tuning, lazy kernel attributes); then the two paths alternate --iters times
(the one that goes first alternates too), each call timed on the host between two device synchronisations.  Reports median, p10,
p90 and p99 ms per call and kernel launches per call.  --trace reads a rocprofv3 --kernel-trace CSV of a run of this tool and adds
the median duration of region_reduce_kernel and of grd.cached_desc (the gather_channels_kernel dispatches of one 1-D row per pair:
grids of at most 4 workgroups in x).
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORK = [   # name, variant, queries, tiles per query, tile pool
    ("vigor_prior180_32x4", "vigor_ori_prior", 32, 4, 32),
    ("vigor_prior180_1x2", "vigor_ori_prior", 1, 2, 2),
    ("oxford_1x4", "oxford", 1, 4, 4),
]


def make(variant, dev):
    from ccvpe_amd import models, weights
    m = models.CVM_VIGOR_ori_prior(dev, 180.0, True) if variant == "vigor_ori_prior" else models.CVM_OxfordRobotCar(dev)
    m.load_state_dict(weights.generate_state_dict(variant, 0))
    return m.to(dev).eval()


def summarize_trace(path: str) -> dict:
    files = [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
    red, gat = [], []
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row.get("Kernel_Name", "")
                dur = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3   # ns -> us
                if "region_reduce_kernel" in name:
                    red.append(dur)
                elif "gather_channels_kernel" in name:
                    gx = int(row.get("Grid_Size_X", row.get("Grid_Size", "0")) or 0)
                    wx = int(row.get("Workgroup_Size_X", row.get("Workgroup_Size", "256")) or 256)
                    if 0 < gx // max(wx, 1) <= 4:
                        gat.append(dur)
    out = {"trace_files": [os.path.relpath(f, ROOT) if f.startswith(ROOT) else os.path.basename(f) for f in files]}
    for k, v in (("region_reduce_kernel", red), ("grd.cached_desc", gat)):
        if v:
            out[k] = {"dispatches": len(v), "median_us": round(float(np.median(v)), 2), "p90_us": round(float(np.percentile(v, 90)), 2)}
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_time_region.json"))
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", default=None)
    args = ap.parse_args()
    if args.trace:
        res = json.load(open(args.out)) if os.path.exists(args.out) else {}
        res["kernels"] = summarize_trace(args.trace)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
        print(json.dumps(res["kernels"]))
        return 0
    import torch
    from ccvpe_amd import _lib, weights
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    models_ = {}
    cases = []
    for name, variant, G, per, pool in WORK:
        if variant not in models_:
            models_[variant] = make(variant, dev)
        m = models_[variant]
        g, _ = weights.generate_inputs(variant, G, 1, 360.0)
        _, s = weights.generate_inputs(variant, pool, 2, 360.0)
        grd, sat = torch.from_numpy(g).to(dev), torch.from_numpy(s).to(dev)
        sc = m.encode_aerial(sat)
        lists = [[int(t) for t in rng.choice(pool, size=per, replace=False)] for _ in range(G)]
        flat = np.asarray([t for l in lists for t in l], dtype=np.int32)

        def path_a(m=m, grd=grd, sc=sc, flat=flat, per=per):
            return m.localize_cached(grd.repeat_interleave(per, 0), sc, tile_index=flat)

        def path_b(m=m, grd=grd, sc=sc, lists=lists):
            return m.localize_region(m.encode_ground(grd), sc, lists)

        cases.append((name, G, per, {"A_repeat_localize_cached": path_a, "B_encode_ground_region": path_b}))

    agree = {}
    for name, G, per, paths in cases:
        for _ in range(args.warmup):
            a = paths["A_repeat_localize_cached"]()
            b = paths["B_encode_ground_region"]()
        torch.cuda.synchronize()
        # the per-pair rows of both paths: the same model, different ground-encoder batches (not bitwise)
        agree[name] = {"pairs": G * per, "same_pair_index": int((a[:, 0] == b["pair_rows"][:, 0]).sum().item()),
                       "max_abs_pair_prob_diff": float((a[:, 1] - b["pair_rows"][:, 1]).abs().max().item())}

    def timed(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return (t1 - t0) * 1e3, int(lib.ccvpe_launch_count() - n0)

    out = {"tool": "tools/time_region.py", "iters": args.iters, "device": torch.cuda.get_device_name(dev), "micro_batch": 32, "cases": {}}
    for name, G, per, paths in cases:
        names = list(paths)
        ms = {k: [] for k in names}
        launches = {k: 0 for k in names}
        for i in range(args.iters):
            for k in (names if i % 2 == 0 else names[::-1]):
                t, n = timed(paths[k])
                ms[k].append(t)
                launches[k] = n
        res = {"queries": G, "tiles_per_query": per, **agree[name]}
        for k in names:
            a = np.asarray(ms[k])
            res[k] = {"median_ms": round(float(np.median(a)), 3), "p10_ms": round(float(np.percentile(a, 10)), 3),
                      "p90_ms": round(float(np.percentile(a, 90)), 3), "p99_ms": round(float(np.percentile(a, 99)), 3),
                      "launches_per_call": launches[k]}
        res["speedup_A_over_B"] = round(res[names[0]]["median_ms"] / res[names[1]]["median_ms"], 3)
        out["cases"][name] = res
    if os.path.exists(args.out):   # keep a kernel summary added earlier
        try:
            prev = json.load(open(args.out))
            if "kernels" in prev:
                out["kernels"] = prev["kernels"]
        except (OSError, ValueError):
            pass
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
