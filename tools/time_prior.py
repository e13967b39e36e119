"""Pose-only forms with a position prior against the same forms without one, in one process (ccvpe_localize_prior).

    python tools/time_prior.py [--iters 50] [--warmup 5] [--out FILE]

Models and inputs are built as bench.py builds them (weights.generate_state_dict(variant, 0), weights.generate_inputs).  Cases: batch 32
and batch 1 of vigor_samearea_fov360_b32 at k = 0 (localize against localize_prior) and k = 8, r = 16 (localize_topk against
localize_prior), and batch 1 of oxford_stream through the cached forms (localize_cached against localize_prior_cached).  The prior is a
Gaussian per query (aerial.gaussian_log_prior, sigma 40 px), made once before timing.  Every shape is warmed up first; then the plain and
the prior form alternate --iters times per case (the one that goes first alternates too), each call timed on the host between two device
synchronisations.  Prints one JSON line: per case and form the median / p50 / p99 ms per call, kernel launches per call
(ccvpe_launch_count delta; the prior adds none), the prior's cost in ms and percent, and whether a zero prior returned the plain rows
bit for bit.
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
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    from ccvpe_amd import _lib, aerial, weights
    lib = _lib.load()
    dev = torch.device("cuda", 0)

    models_ = {}
    cases = []
    for case, wl, batch, k, cached in (("vigor_b32_k0", "vigor_samearea_fov360_b32", 32, 0, False),
                                       ("vigor_b32_k8", "vigor_samearea_fov360_b32", 32, 8, False),
                                       ("vigor_b1_k0", "vigor_samearea_fov360_b32", 1, 0, False),
                                       ("vigor_b1_k8", "vigor_samearea_fov360_b32", 1, 8, False),
                                       ("oxford_stream_b1_cached_k0", "oxford_stream", 1, 0, True)):
        variant, kw, fov = WORKLOADS[wl]
        if wl not in models_:
            models_[wl] = build_model(variant, kw, dev)
        m = models_[wl]
        g, s = weights.generate_inputs(variant, batch, 0, fov)
        g, s = torch.from_numpy(g).to(dev), torch.from_numpy(s).to(dev)
        centres = np.random.default_rng(batch).uniform(100, 412, size=(batch, 2))
        lp = aerial.gaussian_log_prior(centres, 40.0, dev)
        zero = torch.zeros_like(lp)
        r = 16 if k else 0
        if cached:
            cache = m.encode_aerial(s)
            plain = lambda m=m, g=g, c=cache: m.localize_cached(g, c)
            prior = lambda p=lp, m=m, g=g, c=cache: m.localize_prior_cached(g, c, p)
            zrows = lambda m=m, g=g, c=cache, z=zero: m.localize_prior_cached(g, c, z)
        elif k:
            plain = lambda m=m, g=g, s=s, k=k, r=r: m.localize_topk(g, s, k, r)
            prior = lambda p=lp, m=m, g=g, s=s, k=k, r=r: m.localize_prior(g, s, p, k, r)
            zrows = lambda m=m, g=g, s=s, k=k, r=r, z=zero: m.localize_prior(g, s, z, k, r)
        else:
            plain = lambda m=m, g=g, s=s: m.localize(g, s)
            prior = lambda p=lp, m=m, g=g, s=s: m.localize_prior(g, s, p)
            zrows = lambda m=m, g=g, s=s, z=zero: m.localize_prior(g, s, z)
        cases.append((case, wl, batch, k, r, {"plain": plain, "prior": prior}, zrows))

    # warm up every shape (plans, lazy kernel attributes) before anything is timed
    same = {}
    for case, _, _, _, _, paths, zrows in cases:
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        same[case] = bool(torch.equal(paths["plain"](), zrows()))
        torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return (t1 - t0) * 1e3, int(lib.ccvpe_launch_count() - n0)

    out = {"tool": "tools/time_prior.py", "iters": args.iters, "device": torch.cuda.get_device_name(dev), "cases": {}}
    for case, wl, batch, k, r, paths, _ in cases:
        names = list(paths)
        ms = {n: [] for n in names}
        launches = {n: 0 for n in names}
        for i in range(args.iters):
            for n in (names if i % 2 == 0 else names[::-1]):
                t, c = timed(paths[n])
                ms[n].append(t)
                launches[n] = c
        res = {"workload": wl, "batch": batch, "k": k, "radius": r, "zero_prior_rows_equal": same[case]}
        for n in names:
            a = np.asarray(ms[n])
            res[n] = {"median_ms": round(float(np.median(a)), 4), "p50_ms": round(float(np.percentile(a, 50)), 4),
                      "p99_ms": round(float(np.percentile(a, 99)), 4), "launches_per_call": launches[n]}
        pm, qm = res["plain"]["median_ms"], res["prior"]["median_ms"]
        res["prior_cost_ms"] = round(qm - pm, 4)
        res["prior_cost_pct"] = round(100.0 * (qm - pm) / pm, 3)
        res["same_launch_count"] = launches["plain"] == launches["prior"]
        out["cases"][case] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
