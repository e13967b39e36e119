"""Top-K pose hypotheses against the argmax pose, in one process (ccvpe_localize_topk).

    python tools/time_topk.py [--iters 50] [--warmup 5] [--k 8] [--radius 16]

Models and inputs are built as bench.py builds them (weights.generate_state_dict(variant, 0), weights.generate_inputs).  Every shape is
warmed up first; then the two paths alternate --iters times per case (the one that goes first alternates too), each call timed on the
host between two device synchronisations.  Cases: localize against localize_topk(k, radius) at batch 32 and batch 1 of
vigor_samearea_fov360_b32 and at batch 1 of oxford_stream through the cached forms (localize_cached against localize_topk_cached), and
postprocess_rows against postprocess_topk on the forward outputs of the batch-32 case.  Prints one JSON line: per case and path the
median / p50 / p99 ms per call, queries/s at the median, kernel launches per call (ccvpe_launch_count delta), the top-K path's extra
time, and whether row 0 of the top-K rows equals the argmax row.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {   # bench.py WORKLOADS entries used here: (variant, ctor kwargs, fov)
    "vigor_samearea_fov360_b32": ("vigor_ori_prior", dict(ori_noise=180.0, circular_padding=True), 360.0),
    "oxford_stream": ("oxford", {}, 360.0),
}


def build_model(variant, kw, dev):
    from ccvpe_amd import models, weights
    cls = {"vigor_ori_prior": models.CVM_VIGOR_ori_prior, "oxford": models.CVM_OxfordRobotCar}[variant]
    m = cls(dev, kw["ori_noise"], kw["circular_padding"]) if variant == "vigor_ori_prior" else cls(dev)
    m.load_state_dict(weights.generate_state_dict(variant, 0))
    return m.to(dev).eval()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--radius", type=int, default=16)
    args = ap.parse_args()
    import torch
    from ccvpe_amd import _lib, weights
    lib = _lib.load()
    dev = torch.device("cuda", 0)

    models_ = {}
    cases = []
    for case, wl, batch, cached in (("vigor_b32", "vigor_samearea_fov360_b32", 32, False),
                                    ("vigor_b1", "vigor_samearea_fov360_b32", 1, False),
                                    ("oxford_stream_b1_cached", "oxford_stream", 1, True)):
        variant, kw, fov = WORKLOADS[wl]
        if wl not in models_:
            models_[wl] = build_model(variant, kw, dev)
        m = models_[wl]
        g, s = weights.generate_inputs(variant, batch, 0, fov)
        g, s = torch.from_numpy(g).to(dev), torch.from_numpy(s).to(dev)
        K, R = args.k, args.radius
        if cached:
            cache = m.encode_aerial(s)

            def one(m=m, g=g, cache=cache):
                return m.localize_cached(g, cache)

            def topk(m=m, g=g, cache=cache):
                return m.localize_topk_cached(g, cache, K, R)
        else:
            def one(m=m, g=g, s=s):
                return m.localize(g, s)

            def topk(m=m, g=g, s=s):
                return m.localize_topk(g, s, K, R)
        cases.append((case, wl, batch, {"argmax": one, "topk": topk}))
        if batch == 32:   # post-processing alone, on forward outputs the caller holds
            o = m(g, s)
            heat, ori = o[1].clone(), o[2].clone()
            del o

            def pp_one(m=m, heat=heat, ori=ori):
                return m.postprocess_rows(heat, ori)

            def pp_topk(m=m, heat=heat, ori=ori):
                return m.postprocess_topk(heat, ori, K, R)
            cases.append(("postprocess_b32", wl, batch, {"argmax": pp_one, "topk": pp_topk}))

    # warm up every shape (plans, tuning, lazy kernel attributes) before anything is timed
    same = {}
    for case, _, _, paths in cases:
        for _ in range(args.warmup):
            rows = {k: fn() for k, fn in paths.items()}
        torch.cuda.synchronize()
        same[case] = bool(torch.equal(rows["topk"][:, 0], rows["argmax"]))

    def timed(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return (t1 - t0) * 1e3, int(lib.ccvpe_launch_count() - n0)

    out = {"tool": "tools/time_topk.py", "iters": args.iters, "k": args.k, "radius": args.radius, "device": torch.cuda.get_device_name(dev), "cases": {}}
    for case, wl, batch, paths in cases:
        names = list(paths)
        ms = {k: [] for k in names}
        launches = {k: 0 for k in names}
        for i in range(args.iters):
            for k in (names if i % 2 == 0 else names[::-1]):
                t, n = timed(paths[k])
                ms[k].append(t)
                launches[k] = n
        res = {"workload": wl, "batch": batch, "row0_equals_argmax": same[case]}
        for k in names:
            a = np.asarray(ms[k])
            med = float(np.median(a))
            res[k] = {"median_ms": round(med, 4), "p50_ms": round(float(np.percentile(a, 50)), 4),
                      "p99_ms": round(float(np.percentile(a, 99)), 4), "queries_per_s": round(batch * 1e3 / med, 2),
                      "launches_per_call": launches[k]}
        a1, tk = res["argmax"]["median_ms"], res["topk"]["median_ms"]
        res["topk_extra_ms"] = round(tk - a1, 4)
        res["topk_extra_pct"] = round(100.0 * (tk - a1) / a1, 2)
        out["cases"][case] = res
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
