"""The heading prior (ccvpe_localize_heading_prior*) against the heading forms it extends and against the detour through
the full forward's outputs, in one process.

    python tools/time_heading_prior.py [--iters 40] [--warmup 5] [--radius 8] [--bins 72] [--out profiles/time_heading_prior.json]

Models and inputs are built as bench.py builds them (weights.generate_state_dict(variant, 0), weights.generate_inputs).  Cases: batch 1
of oxford_stream through the cached forms, batch 1 and batch 32 of vigor_samearea_fov360_b32 through the full forms, each with a
Gaussian position log-prior and a von Mises heading prior per query.  Per case three forms:

    a  heading        localize_heading_cached / localize_heading with the position prior
    b  heading_prior  localize_heading_prior_cached / localize_heading_prior with both priors
    c  detour         forward_cached / forward, then heading_prior_map and postprocess_heading over its outputs

and, for the kernels alone, heading_prior_map (with and without a position prior) and heading_predict.

Every shape is warmed up first; then the forms alternate --iters times per case (the order rotates), each call timed on the host
between two device synchronisations.  Prints one JSON line: per case and form the median / p99 ms per call and the library's kernel
launches per call (ccvpe_launch_count delta), the price of the feature b - a, the ratio c / b, and whether b and c returned the same
bits.
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
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--bins", type=int, default=72)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    from ccvpe_amd import _lib, aerial, weights
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    R, NB = args.radius, args.bins

    models_ = {}
    cases = []
    for case, wl, batch, cached in (("oxford_stream_b1_cached", "oxford_stream", 1, True),
                                    ("vigor_b1", "vigor_samearea_fov360_b32", 1, False),
                                    ("vigor_b32", "vigor_samearea_fov360_b32", 32, False)):
        variant, kw, fov = WORKLOADS[wl]
        if wl not in models_:
            models_[wl] = build_model(variant, kw, dev)
        m = models_[wl]
        g, s = weights.generate_inputs(variant, batch, 0, fov)
        g, s = torch.from_numpy(g).to(dev), torch.from_numpy(s).to(dev)
        cache = m.encode_aerial(s) if cached else None
        rng = np.random.default_rng(1)
        lp = aerial.gaussian_log_prior(rng.uniform(100, 412, size=(batch, 2)), 40.0, dev)
        tb = torch.from_numpy(aerial.von_mises_heading_log_prior(rng.uniform(0.0, 360.0, size=batch), np.full(batch, 8.0), NB)).to(dev)
        fwd = m.forward_cached(g, cache) if cached else m(g, s)
        ori = fwd[2]
        hist = torch.rand(batch, NB, device=dev)
        taps = torch.from_numpy(aerial.gaussian_taps(2.0, 6)).to(dev)
        turn, floor = torch.zeros(batch, device=dev), torch.full((batch,), 1e-3, device=dev)

        def heading(m=m, g=g, s=s, c=cache, lp=lp):
            return (m.localize_heading_cached(g, c, lp, radius=R, bins=NB, summary=True) if c is not None
                    else m.localize_heading(g, s, lp, radius=R, bins=NB, summary=True))

        def heading_prior(m=m, g=g, s=s, c=cache, lp=lp, tb=tb):
            return (m.localize_heading_prior_cached(g, c, tb, lp, radius=R, bins=NB, summary=True) if c is not None
                    else m.localize_heading_prior(g, s, tb, lp, radius=R, bins=NB, summary=True))

        def detour(m=m, g=g, s=s, c=cache, lp=lp, tb=tb):
            out = m.forward_cached(g, c) if c is not None else m(g, s)
            return m.postprocess_heading(out[0], out[2], m.heading_prior_map(out[2], tb, lp), radius=R, bins=NB, summary=True)

        paths = {"heading": heading, "heading_prior": heading_prior, "detour": detour,
                 "kernel_map_prior": lambda m=m, o=ori, tb=tb, lp=lp: m.heading_prior_map(o, tb, lp),
                 "kernel_map": lambda m=m, o=ori, tb=tb: m.heading_prior_map(o, tb),
                 "kernel_predict": lambda m=m, h=hist, t=turn, tp=taps, f=floor: m.heading_predict(h, t, tp, f)}
        cases.append((case, wl, batch, paths))

    same = {}
    for case, _, _, paths in cases:
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        a, b = paths["heading_prior"](), paths["detour"]()
        same[case] = all(bool(torch.equal(x.view(torch.int32), y.view(torch.int32))) for x, y in zip(a, b))
        torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return (t1 - t0) * 1e3, int(lib.ccvpe_launch_count() - n0)

    out = {"tool": "tools/time_heading_prior.py", "iters": args.iters, "radius": R, "bins": NB, "device": torch.cuda.get_device_name(dev),
           "cases": {}}
    for case, wl, batch, paths in cases:
        names = list(paths)
        ms = {n: [] for n in names}
        launches = {n: 0 for n in names}
        for i in range(args.iters):
            k = i % len(names)
            for n in names[k:] + names[:k]:
                t, c = timed(paths[n])
                ms[n].append(t)
                launches[n] = c
        res = {"workload": wl, "batch": batch, "heading_prior_equals_detour_bits": same[case]}
        for n in names:
            a = np.asarray(ms[n])
            res[n] = {"median_ms": round(float(np.median(a)), 4), "p99_ms": round(float(np.percentile(a, 99)), 4),
                      "library_launches_per_call": launches[n]}
        a, b, c = (res[n]["median_ms"] for n in ("heading", "heading_prior", "detour"))
        res["heading_prior_cost_ms"] = round(b - a, 4)
        res["heading_prior_cost_pct"] = round(100.0 * (b - a) / a, 3)
        res["detour_over_heading_prior"] = round(c / b, 3)
        out["cases"][case] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
