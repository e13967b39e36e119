"""The link statistics of a recorded stream (motion.link_stream, ccvpe_track_link) against the same sums written in torch -
what a caller has to do without it - in one process.

    python tools/time_link.py [--frames 100] [--iters 6] [--warmup 1] [--torch-links 2] [--out profiles/time_link.json]

The log is tools/time_smooth.py's synthetic one (no network runs), swept once by smooth.smooth_stream outside the timing.  Cases: radius 6
(sigma 2 px) and radius 32 (sigma 11 px), batch 1 and batch 32, --frames frames each.  Forms:

    a  library   motion.link_stream(model, log, maps): every link of the stream
    b  torch     per link: tools/time_smooth.py's prior and the divide for g, then D by the faster of two routes, chosen per case on one
                 link - `products`: one shifted product and sum per offset, (2r + 2)^2 of them; `unfold`: per row offset one einsum of g
                 with the unfolded view of the shifted rows of b, 2r + 2 of them - the weights, M, J and Z
                 timed over --torch-links links only and reported per link: at radius 32 a whole sweep of it runs for minutes

Every shape is warmed up first; then the two forms alternate --iters times per case (the order rotates), each timed on the host between
two device synchronisations; the whole measurement runs twice.  Prints one JSON line: per case, run and form the median / p99 ms per
link, the library's launches per link, the ratio b / a, the largest relative difference between the two forms' moves on one link where
they are above 1e-9 of the largest, and the library form's compulsory traffic per link and query - five map passes of 1 MB (b, s' read
and g written; b, g read) and the tile sums written and read once, 2 * 256 * (2r + 2)^2 * 4 bytes - as a rate against the copy rate
of tools/ubench_hbm.py.  How the library's time splits between its launches is not visible from the host: a kernel trace of one call
shows it (DESIGN.md 4.25 records one).
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import time_smooth  # noqa: E402  (the synthetic log and the prior in torch)

FLOOR, SHIFT = time_smooth.FLOOR, time_smooth.SHIFT
CASES = ((6, 2.0), (32, 11.0))      # (radius, sigma)
MAP_BYTES = 4 * 512 * 512
HBM_COPY_TBPS = time_smooth.HBM_COPY_TBPS


def torch_link(belief, nxt, shift, taps, floor, route):
    """(moves [B,K,K], stats [B,4]) of one link in torch ops; one shift for the batch"""
    import torch
    import torch.nn.functional as F
    B = belief.shape[0]
    r = taps.numel() - 1
    K = 2 * r + 2
    prior = time_smooth.torch_predict_c(belief, shift, taps) + floor
    g = torch.where(nxt > 0, nxt / prior, torch.zeros_like(nxt))
    dx, dy = float(shift[0]), float(shift[1])
    ix, iy = int(np.floor(dx)), int(np.floor(dy))
    fx, fy = dx - ix, dy - iy
    # pad[.., P + y, P + x] = b[y, x]; source = target - i - r - 1 + k
    P = 600 + r + 1
    pad = F.pad(belief, (P, P, P, P))
    y0, x0 = P - iy - r - 1, P - ix - r - 1
    if route == "products":
        D = torch.stack([torch.stack([(g * pad[:, y0 + ky:y0 + ky + 512, x0 + kx:x0 + kx + 512]).sum(dim=(1, 2)) for kx in range(K)], dim=1)
                         for ky in range(K)], dim=1)
    else:
        rows = []
        for ky in range(K):
            win = pad[:, y0 + ky:y0 + ky + 512, x0:x0 + 512 + K - 1].unfold(2, 512, 1)      # [B, 512, K, 512], a view
            rows.append(torch.einsum("byx,bykx->bk", g, win))
        D = torch.stack(rows, dim=1)
    t = torch.cat([taps, taps.new_zeros(1)])
    k = torch.arange(K, device=taps.device)
    ta, tc = t[(k - r).abs().clamp(max=r + 1)], t[(k - 1 - r).abs().clamp(max=r + 1)]
    ux, uy = fx * ta + (1 - fx) * tc, fy * ta + (1 - fy) * tc
    moves = (uy[:, None] * ux[None, :]) * D
    M, G, Sb = moves.sum(dim=(1, 2)), g.view(B, -1).sum(dim=1), belief.view(B, -1).sum(dim=1)
    J = floor * G * Sb
    return moves, torch.stack([M + J, G, J, M], dim=1)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--torch-links", type=int, default=2)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    from ccvpe_amd import _lib, aerial, models, motion, smooth, weights
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    model = models.CVM_OxfordRobotCar(dev)
    model.load_state_dict(weights.generate_state_dict("oxford", 0))
    model = model.to(dev).eval()

    def timed(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        del res
        return (t1 - t0) * 1e3, int(lib.ccvpe_launch_count() - n0)

    out = {"tool": "tools/time_link.py", "frames": args.frames, "iters": args.iters, "torch_links": args.torch_links,
           "device": torch.cuda.get_device_name(dev), "floor": FLOOR, "shift_px": list(SHIFT), "hbm_copy_TBps": HBM_COPY_TBPS, "cases": {}}
    for radius, sigma in CASES:
        taps = torch.as_tensor(aerial.gaussian_taps(sigma, radius)).to(dev)
        for batch in args.batches:
            log = time_smooth.synthetic_log(args.frames, batch, taps, dev)
            maps, _ = smooth.smooth_stream(model, log)
            links = len(log) - 1
            tl = min(args.torch_links, links)

            def library(log=log, maps=maps):
                return motion.link_stream(model, log, maps)

            def torch_form(route, log=log, maps=maps, tl=tl):
                return [torch_link(log[t][0], maps[t + 1], SHIFT, taps, FLOOR, route) for t in range(tl)]

            # the faster torch route, on one link (after one untimed call each); products only where it is a few hundred launches
            routes = ["unfold"] + (["products"] if radius <= 6 else [])
            cost = {}
            for route in routes:
                torch_link(log[0][0], maps[1], SHIFT, taps, FLOOR, route)
                cost[route] = min(timed(lambda: torch_link(log[0][0], maps[1], SHIFT, taps, FLOOR, route))[0] for _ in range(2))
            route = min(cost, key=cost.get)
            paths = {"library": (library, links), "torch": (lambda: torch_form(route), tl)}
            for _ in range(args.warmup):
                for fn, _n in paths.values():
                    fn()
            a, b = library()[0][0], torch_link(log[0][0], maps[1], SHIFT, taps, FLOOR, route)[0]
            big = b > 1e-9 * b.max()
            diff = float(((a - b).abs()[big] / b[big]).max().item())
            del a, b, big
            torch.cuda.synchronize()
            res = {"radius": radius, "batch": batch, "torch_route": route, "torch_route_ms_one_link": {k: round(v, 4) for k, v in cost.items()},
                   "library_against_torch_max_rel_diff_link0": diff, "runs": []}
            names = list(paths)
            for run in range(2):
                ms = {n: [] for n in names}
                launches = {n: 0 for n in names}
                for i in range(args.iters):
                    k = i % len(names)
                    for n in names[k:] + names[:k]:
                        t, c = timed(paths[n][0])
                        ms[n].append(t / paths[n][1])
                        launches[n] = c / paths[n][1]
                r = {}
                for n in names:
                    v = np.asarray(ms[n])
                    r[n] = {"per_link_median_ms": round(float(np.median(v)), 5), "per_link_p99_ms": round(float(np.percentile(v, 99)), 5),
                            "library_launches_per_link": launches[n]}
                r["torch_over_library"] = round(r["torch"]["per_link_median_ms"] / r["library"]["per_link_median_ms"], 3)
                bytes_per_link = (5 * MAP_BYTES + 2 * 256 * (2 * radius + 2) ** 2 * 4) * batch
                rate = bytes_per_link / (r["library"]["per_link_median_ms"] * 1e-3) / 1e12
                r["library_bytes_per_link"] = bytes_per_link
                r["library_TBps"] = round(rate, 4)
                r["library_share_of_hbm_copy_rate"] = round(rate / HBM_COPY_TBPS, 4)
                res["runs"].append(r)
            out["cases"][f"r{radius}_b{batch}"] = res
            del log, maps
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
