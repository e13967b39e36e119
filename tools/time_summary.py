"""The posterior summary (ccvpe_localize_summary*) against the update forms it extends and against what a caller has to
do without it, in one process.

    python tools/time_summary.py [--iters 40] [--warmup 5] [--radius 8] [--out profiles/time_summary.json]

Models and inputs are built as bench.py builds them (weights.generate_state_dict(variant, 0), weights.generate_inputs).  Cases: batch 1
of oxford_stream through the cached forms, batch 1 and batch 32 of vigor_samearea_fov360_b32 through the full forms, each with a
Gaussian log-prior.  Per case four forms:

    a  update        track_update_cached / track_update: rows and the posterior map
    b  summary_map   localize_summary_cached / localize_summary with posterior=True: rows, summary and the map
    b' summary       the same without the map
    c  torch         a, then the same 16 numbers from the map in torch ops (float64 sums, the window sliced around the argmax)

Every shape is warmed up first; then the forms alternate --iters times per case (the order rotates), each call timed on the host
between two device synchronisations.  Prints one JSON line: per case and form the median / p99 ms per call and the library's kernel
launches per call (ccvpe_launch_count delta; torch's own launches are not counted), the summary's cost b - a and b' - a, the ratio
c / b, and the largest difference between the device's and torch's 16 numbers.
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


def torch_summary(post, radius):
    """the 16 numbers of every map of post [B, 512, 512] in torch ops: float64 sums over the map, then the window of each query"""
    import torch
    B = post.shape[0]
    h = post.view(B, -1).double()
    ar = torch.arange(512, dtype=torch.float64, device=post.device)
    x, y = ar.repeat(512), ar.repeat_interleave(512)

    def moments(w, xs, ys):
        s = w.sum(-1)
        mx, my = (w * xs).sum(-1) / s, (w * ys).sum(-1) / s
        return [s, mx, my, (w * xs * xs).sum(-1) / s - mx * mx, (w * xs * ys).sum(-1) / s - mx * my, (w * ys * ys).sum(-1) / s - my * my]

    prob, idx = post.view(B, -1).max(dim=1)
    s0, mx, my, vxx, vxy, vyy = moments(h, x, y)
    p = h / s0[:, None]
    ent = -(torch.where(p > 0, p * torch.log(torch.where(p > 0, p, torch.ones_like(p))), torch.zeros_like(p))).sum(-1)
    cols = [idx.double(), prob.double(), s0, ent, mx, my, vxx, vxy, vyy]
    win = []
    for b, i in enumerate(idx.tolist()):          # (the argmax comes back to the host: the window's bounds depend on it)
        ys_, xs_ = divmod(i, 512)
        y0, y1, x0, x1 = max(ys_ - radius, 0), min(ys_ + radius, 511) + 1, max(xs_ - radius, 0), min(xs_ + radius, 511) + 1
        w = post[b, y0:y1, x0:x1].double().reshape(-1)
        wx = ar[x0:x1].repeat(y1 - y0)
        wy = ar[y0:y1].repeat_interleave(x1 - x0)
        m = moments(w, wx, wy)
        win.append(torch.stack([m[0] / s0[b], *m[1:], torch.tensor(float((y1 - y0) * (x1 - x0)), dtype=torch.float64, device=post.device)]))
    return torch.cat([torch.stack(cols, dim=1), torch.stack(win)], dim=1).float()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    from ccvpe_amd import _lib, aerial, weights
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    R = args.radius

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
        centres = np.random.default_rng(1).uniform(100, 412, size=(batch, 2))
        lp = aerial.gaussian_log_prior(centres, 40.0, dev)

        def update(m=m, g=g, s=s, c=cache, lp=lp):
            return m.track_update_cached(g, c, lp) if c is not None else m.track_update(g, s, lp)

        def summary_map(m=m, g=g, s=s, c=cache, lp=lp):
            return (m.localize_summary_cached(g, c, lp, radius=R, posterior=True) if c is not None
                    else m.localize_summary(g, s, lp, radius=R, posterior=True))

        def summary(m=m, g=g, s=s, c=cache, lp=lp):
            return m.localize_summary_cached(g, c, lp, radius=R) if c is not None else m.localize_summary(g, s, lp, radius=R)

        def torch_form(update=update):
            rows, post = update()
            return rows, torch_summary(post, R), post

        cases.append((case, wl, batch, {"update": update, "summary_map": summary_map, "summary": summary, "torch": torch_form}))

    diff = {}
    for case, _, _, paths in cases:
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        a, b = paths["summary_map"]()[1].double(), paths["torch"]()[1].double()
        diff[case] = float(((a - b).abs() / b.abs().clamp(min=1.0)).max().item())
        torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return (t1 - t0) * 1e3, int(lib.ccvpe_launch_count() - n0)

    out = {"tool": "tools/time_summary.py", "iters": args.iters, "radius": R, "device": torch.cuda.get_device_name(dev), "cases": {}}
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
        res = {"workload": wl, "batch": batch, "max_scaled_difference_device_vs_torch": diff[case]}
        for n in names:
            a = np.asarray(ms[n])
            res[n] = {"median_ms": round(float(np.median(a)), 4), "p99_ms": round(float(np.percentile(a, 99)), 4),
                      "library_launches_per_call": launches[n]}
        a, b, b1, c = (res[n]["median_ms"] for n in ("update", "summary_map", "summary", "torch"))
        res["summary_map_cost_ms"] = round(b - a, 4)
        res["summary_cost_ms"] = round(b1 - a, 4)
        res["summary_map_cost_pct"] = round(100.0 * (b - a) / a, 3)
        res["torch_over_summary_map"] = round(c / b, 3)
        out["cases"][case] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
