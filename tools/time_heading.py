"""The heading posterior (ccvpe_localize_heading*) against the summary forms it extends and against what a caller has to
do without it, in one process.

    python tools/time_heading.py [--iters 40] [--warmup 5] [--radius 8] [--bins 72] [--out profiles/time_heading.json]

Models and inputs are built as bench.py builds them (weights.generate_state_dict(variant, 0), weights.generate_inputs).  Cases: batch 1
of oxford_stream through the cached forms, batch 1 and batch 32 of vigor_samearea_fov360_b32 through the full forms, each with a
Gaussian log-prior.  Per case three forms:

    a  summary   localize_summary_cached / localize_summary: rows and the summary
    b  heading   localize_heading_cached / localize_heading with summary=True: rows, heading, hist and the summary
    c  torch     forward_cached / forward, then the 12 + bins heading numbers in torch ops: softmax(logits + prior), acos, bucketize by
                 multiplication, scatter_add (float atomics: its bits depend on scheduling), float64 moments, the window sliced around
                 the argmax

and, for the kernel alone, postprocess_heading against postprocess_summary over the forward's outputs with the network's field, a
constant field (every lane of a wave in one bin) and a random one (every lane in another).

Every shape is warmed up first; then the forms alternate --iters times per case (the order rotates), each call timed on the host
between two device synchronisations.  Prints one JSON line: per case and form the median / p99 ms per call and the library's kernel
launches per call (ccvpe_launch_count delta; torch's own launches are not counted), the heading's cost b - a, the ratio c / b, and the
largest difference between the device's and torch's numbers.
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


def torch_heading(logits, ori, lp, radius, bins):
    """(heading [B, 12], hist [B, bins]) from forward outputs in torch ops"""
    import torch
    B = logits.shape[0]
    post = torch.softmax(logits + lp.reshape(B, -1), dim=1)
    c, s = ori[:, 0].reshape(B, -1), ori[:, 1].reshape(B, -1)
    valid = torch.isfinite(c) & torch.isfinite(s) & ~((c == 0) & (s == 0))
    ang = torch.rad2deg(torch.acos(c.clamp(-1.0, 1.0)))
    ang = torch.where(s < 0, 360.0 - ang, ang)
    b = (ang * (bins / 360.0)).long().clamp(0, bins)
    b = torch.where(b >= bins, b - bins, b)
    h = torch.where(valid, post, torch.zeros_like(post))
    hist = torch.zeros(B, bins, dtype=torch.float32, device=logits.device).scatter_add_(1, torch.where(valid, b, torch.zeros_like(b)), h)
    hd, cd, sd = h.double(), torch.where(valid, c, torch.zeros_like(c)).double(), torch.where(valid, s, torch.zeros_like(s)).double()

    def moments(w, cc, ss):
        M = w.sum(-1)
        C, S = (w * cc).sum(-1) / M, (w * ss).sum(-1) / M
        R = torch.sqrt(C * C + S * S)
        return [M, C, S, torch.rad2deg(torch.atan2(S, C)) % 360.0, R]

    cols = moments(hd, cd, sd)
    mode = hist.argmax(dim=1)
    cols += [mode.double(), hist.gather(1, mode[:, None])[:, 0].double() / cols[0]]
    win = []
    for q, i in enumerate(post.argmax(dim=1).tolist()):          # (the argmax comes back to the host: the window's bounds depend on it)
        ys_, xs_ = divmod(i, 512)
        y0, y1, x0, x1 = max(ys_ - radius, 0), min(ys_ + radius, 511) + 1, max(xs_ - radius, 0), min(xs_ + radius, 511) + 1
        sl = (q, slice(y0, y1), slice(x0, x1))
        win.append(torch.stack(moments(hd.view(B, 512, 512)[sl].reshape(-1), cd.view(B, 512, 512)[sl].reshape(-1),
                                       sd.view(B, 512, 512)[sl].reshape(-1))))
    return torch.cat([torch.stack(cols, dim=1), torch.stack(win)], dim=1).float(), hist


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
        centres = np.random.default_rng(1).uniform(100, 412, size=(batch, 2))
        lp = aerial.gaussian_log_prior(centres, 40.0, dev)
        fwd = m.forward_cached(g, cache) if cached else m(g, s)
        logits, ori = fwd[0], fwd[2]
        ang = torch.rand(batch, 512, 512, device=dev) * (2.0 * np.pi)
        fields = {"network": ori, "constant": torch.stack([torch.full_like(ang, 0.6), torch.full_like(ang, 0.8)], dim=1).contiguous(),
                  "random": torch.stack([torch.cos(ang), torch.sin(ang)], dim=1).contiguous()}

        def summary(m=m, g=g, s=s, c=cache, lp=lp):
            return m.localize_summary_cached(g, c, lp, radius=R) if c is not None else m.localize_summary(g, s, lp, radius=R)

        def heading(m=m, g=g, s=s, c=cache, lp=lp):
            return (m.localize_heading_cached(g, c, lp, radius=R, bins=NB, summary=True) if c is not None
                    else m.localize_heading(g, s, lp, radius=R, bins=NB, summary=True))

        def torch_form(m=m, g=g, s=s, c=cache, lp=lp):
            out = m.forward_cached(g, c) if c is not None else m(g, s)
            return torch_heading(out[0], out[2], lp, R, NB)

        paths = {"summary": summary, "heading": heading, "torch": torch_form,
                 "kernel_summary": lambda m=m, lg=logits, o=ori, lp=lp: m.postprocess_summary(lg, o, lp, radius=R)}
        for fname, f in fields.items():
            paths["kernel_heading_" + fname] = lambda m=m, lg=logits, o=f, lp=lp: m.postprocess_heading(lg, o, lp, radius=R, bins=NB, summary=True)
        cases.append((case, wl, batch, paths))

    diff = {}
    for case, _, _, paths in cases:
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        dev_out, ref = paths["heading"](), paths["torch"]()
        a, b = dev_out[1].double(), ref[0].double()
        diff[case] = {"heading": float(((a - b).abs() / b.abs().clamp(min=1.0)).max().item()),
                      "hist": float((dev_out[2].double() - ref[1].double()).abs().max().item())}
        torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return (t1 - t0) * 1e3, int(lib.ccvpe_launch_count() - n0)

    out = {"tool": "tools/time_heading.py", "iters": args.iters, "radius": R, "bins": NB, "device": torch.cuda.get_device_name(dev), "cases": {}}
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
        res = {"workload": wl, "batch": batch, "max_difference_device_vs_torch": diff[case]}
        for n in names:
            a = np.asarray(ms[n])
            res[n] = {"median_ms": round(float(np.median(a)), 4), "p99_ms": round(float(np.percentile(a, 99)), 4),
                      "library_launches_per_call": launches[n]}
        a, b, c = (res[n]["median_ms"] for n in ("summary", "heading", "torch"))
        res["heading_cost_ms"] = round(b - a, 4)
        res["heading_cost_pct"] = round(100.0 * (b - a) / a, 3)
        res["torch_over_heading"] = round(c / b, 3)
        for fname in ("network", "constant", "random"):
            res["kernel_cost_ms_" + fname] = round(res["kernel_heading_" + fname]["median_ms"] - res["kernel_summary"]["median_ms"], 4)
        out["cases"][case] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
