"""One tracked frame (ccvpe_track_predict + ccvpe_track_update*) against the prior forms it extends and against what a
caller has to do without it, in one process.

    python tools/time_track.py [--iters 40] [--warmup 5] [--out profiles/time_track.json]

Models and inputs are built as bench.py builds them (weights.generate_state_dict(variant, 0), weights.generate_inputs).  Cases: batch 1
of oxford_stream through the cached forms, batch 1 and batch 32 of vigor_samearea_fov360_b32 through the full forms.  Per case three
forms, each returning the frame's rows and leaving the next frame's belief on the device where the form has one:

    a  prior    localize_prior_cached / localize_prior with a ready-made log-prior (no filter: the floor under the other two)
    b  track    track_predict (sigma 2 px, radius 6, floor 1e-9, a fractional shift) + track_update_cached / track_update
    c  torch    the same step with today's entry points: forward_cached / forward, then in torch softmax(logits + prior), argmax and
                gather for the row, and for the next prior a zero-filled bilinear shift (four weighted slices), the two conv2d blur
                passes, add floor, log

Every shape is warmed up first; then the three forms alternate --iters times per case (the order rotates), each call timed on the host
between two device synchronisations.  Prints one JSON line: per case and form the median / p99 ms per call and the library's kernel
launches per call (ccvpe_launch_count delta; torch's own launches are not counted), the filter's cost b - a, the ratio c / b, and
whether b and c name the same pixel.
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
SIGMA, RADIUS, FLOOR = 2.0, 6, 1e-9
SHIFT = (3.37, -1.81)


def build_model(variant, kw, dev):
    from ccvpe_amd import models, weights
    cls = {"vigor_ori_prior": models.CVM_VIGOR_ori_prior, "oxford": models.CVM_OxfordRobotCar}[variant]
    m = cls(dev, kw["ori_noise"], kw["circular_padding"]) if variant == "vigor_ori_prior" else cls(dev)
    m.load_state_dict(weights.generate_state_dict(variant, 0))
    return m.to(dev).eval()


def torch_predict(belief, shift, taps, floor):
    """track_predict in torch ops (one shift for the batch): zero-filled bilinear shift, blur along x then y, log(. + floor)"""
    import torch
    import torch.nn.functional as F
    B = belief.shape[0]
    dx, dy = float(shift[0]), float(shift[1])
    ix, iy = int(np.floor(dx)), int(np.floor(dy))
    fx, fy = dx - ix, dy - iy
    r = taps.numel() - 1
    pad = F.pad(belief.view(B, 1, 512, 512), (513, 513, 513, 513))

    def at(oy, ox):   # the belief moved by (ix + ox, iy + oy) whole pixels
        y0, x0 = 513 - iy - oy, 513 - ix - ox
        return pad[:, :, y0 - r:y0 + 512 + r, x0 - r:x0 + 512 + r]

    s = (1 - fy) * ((1 - fx) * at(0, 0) + fx * at(0, 1)) + fy * ((1 - fx) * at(1, 0) + fx * at(1, 1))
    full = torch.cat([taps.flip(0)[:-1], taps])
    c = F.conv2d(F.conv2d(s, full.view(1, 1, 1, -1)), full.view(1, 1, -1, 1))
    return torch.log(c + floor).view(B, 512, 512)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    from ccvpe_amd import _lib, aerial, weights
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    taps_np = aerial.gaussian_taps(SIGMA, RADIUS)
    taps = torch.as_tensor(taps_np).to(dev)

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
        # the previous frame's belief and a ready-made prior from it
        _, belief = m.track_update_cached(g, cache) if cached else m.track_update(g, s)
        shift = torch.tensor([SHIFT] * batch, dtype=torch.float32, device=dev)
        floor = torch.full((batch,), FLOOR, dtype=torch.float32, device=dev)
        ready = m.track_predict(belief, shift, taps, floor)
        state = {"last": None}

        def prior(m=m, g=g, s=s, c=cache, lp=ready):
            return m.localize_prior_cached(g, c, lp) if c is not None else m.localize_prior(g, s, lp)

        def track(m=m, g=g, s=s, c=cache, bel=belief, sh=shift, fl=floor, st=state):
            lp = m.track_predict(bel, sh, taps, fl)
            rows, st["last"] = m.track_update_cached(g, c, lp) if c is not None else m.track_update(g, s, lp)
            return rows

        def torch_form(m=m, g=g, s=s, c=cache, bel=belief, st=state):
            lp = torch_predict(bel, SHIFT, taps, FLOOR)
            out = m.forward_cached(g, c) if c is not None else m(g, s)
            post = torch.softmax(out[0] + lp.view(lp.shape[0], -1), dim=1)
            prob, idx = post.max(dim=1)
            cs = out[2].view(post.shape[0], 2, -1).gather(2, idx.view(-1, 1, 1).expand(-1, 2, 1))[:, :, 0]
            st["last"] = post
            return torch.cat([idx.to(torch.float32)[:, None], prob[:, None], cs], dim=1)

        cases.append((case, wl, batch, {"prior": prior, "track": track, "torch": torch_form}))

    same = {}
    for case, _, _, paths in cases:
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        same[case] = bool(torch.equal(paths["track"]()[:, 0], paths["torch"]()[:, 0]))
        torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return (t1 - t0) * 1e3, int(lib.ccvpe_launch_count() - n0)

    out = {"tool": "tools/time_track.py", "iters": args.iters, "device": torch.cuda.get_device_name(dev),
           "predict": {"sigma_px": SIGMA, "radius": RADIUS, "floor": FLOOR, "shift_px": list(SHIFT)}, "cases": {}}
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
        res = {"workload": wl, "batch": batch, "track_and_torch_name_the_same_pixel": same[case]}
        for n in names:
            a = np.asarray(ms[n])
            res[n] = {"median_ms": round(float(np.median(a)), 4), "p99_ms": round(float(np.percentile(a, 99)), 4),
                      "library_launches_per_call": launches[n]}
        a, b, c = (res[n]["median_ms"] for n in ("prior", "track", "torch"))
        res["filter_cost_ms"] = round(b - a, 4)
        res["filter_cost_pct"] = round(100.0 * (b - a) / a, 3)
        res["torch_over_track"] = round(c / b, 3)
        out["cases"][case] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
