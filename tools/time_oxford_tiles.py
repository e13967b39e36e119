"""Oxford test loop at batch 32: aerial side per query against per distinct tile (indexed cached forms).

    python tools/time_oxford_tiles.py [--tiles 1,2,4,8,32] [--batch 32] [--iters 30] [--warmup 3]

Synthetic weights (weights.generate_state_dict("oxford", 0)), a synthetic uint8 satellite map resident on the device and a drive of
--batch ground frames over T distinct 800 x 800 windows (consecutive frames share a tile, as the unshuffled test loader gives them).
Two paths per T:
  per_query: aerial.oxford_aerial on every coordinate + localize                       (B aerial encodings)
  per_tile:  aerial.oxford_tiles + oxford_tile_aerial of the T origins + encode_aerial
             + localize_cached(..., tile_index=...)                                    (T aerial encodings)
Every case is warmed up first (plans, tuning, lazy kernel attributes); then the two paths alternate --iters times (the one that goes
first alternates too), each call timed on the host between two device synchronisations.  Prints one JSON line: per T and path the
median / p10 / p90 ms per batch, queries/s at the median and kernel launches per call, and how far the two paths' rows are apart (not
bitwise: the encode plan at batch T may run other tiles than the full plan at batch B).
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

GRID_COLS = 8   # tiles of the synthetic map per row of the 400-px grid


def drive(n_tiles: int, batch: int, rng) -> np.ndarray:
    """batch (col, row) coordinates visiting n_tiles windows in runs of consecutive frames: tile j has origin
    (400 * (1 + j % GRID_COLS), 400 * (1 + j // GRID_COLS)); a coordinate 200 .. 599 px past an origin selects that window"""
    tile = (np.arange(batch) * n_tiles) // batch
    x0 = 400.0 * (1 + tile % GRID_COLS)
    y0 = 400.0 * (1 + tile // GRID_COLS)
    return np.stack([x0 + rng.uniform(200.5, 598.5, batch), y0 + rng.uniform(200.5, 598.5, batch)], axis=1)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tiles", default="1,2,4,8,32")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from ccvpe_amd import _lib, aerial, models, weights
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    B = args.batch
    tiles = [int(t) for t in args.tiles.split(",")]
    rng = np.random.default_rng(0)

    m = models.CVM_OxfordRobotCar(dev)
    m.load_state_dict(weights.generate_state_dict("oxford", 0))
    m.to(dev).eval()
    rows_needed = 1 + (max(tiles) - 1) // GRID_COLS
    mp = torch.from_numpy(rng.integers(0, 256, size=(400 * (rows_needed + 3), 400 * (GRID_COLS + 3), 3), dtype=np.uint8)).to(dev)
    g, _ = weights.generate_inputs("oxford", B, 0, 360.0)
    grd = torch.from_numpy(g).to(dev)

    cases = []
    for T in tiles:
        coords = drive(T, B, rng)
        assert aerial.oxford_tiles(coords)["origin"].shape[0] == T

        def per_query(coords=coords):
            return m.localize(grd, aerial.oxford_aerial(mp, coords))

        def per_tile(coords=coords):
            t = aerial.oxford_tiles(coords)
            cache = m.encode_aerial(aerial.oxford_tile_aerial(mp, t["origin"]))
            return m.localize_cached(grd, cache, tile_index=t["tile_index"])

        cases.append((T, {"per_query": per_query, "per_tile": per_tile}))

    diff = {}
    for T, paths in cases:
        for _ in range(args.warmup):
            rows = {k: fn() for k, fn in paths.items()}
        torch.cuda.synchronize()
        a, b = rows["per_query"], rows["per_tile"]
        diff[T] = {"same_index": int((a[:, 0] == b[:, 0]).sum().item()),
                   "max_abs_prob_diff": float((a[:, 1] - b[:, 1]).abs().max().item())}

    def timed(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return (t1 - t0) * 1e3, int(lib.ccvpe_launch_count() - n0)

    out = {"tool": "tools/time_oxford_tiles.py", "batch": B, "iters": args.iters, "device": torch.cuda.get_device_name(dev), "cases": {}}
    for T, paths in cases:
        names = list(paths)
        ms = {k: [] for k in names}
        launches = {k: 0 for k in names}
        for i in range(args.iters):
            for k in (names if i % 2 == 0 else names[::-1]):
                t, n = timed(paths[k])
                ms[k].append(t)
                launches[k] = n
        res = {"tiles": T, **diff[T]}
        for k in names:
            a = np.asarray(ms[k])
            med = float(np.median(a))
            res[k] = {"median_ms": round(med, 3), "p10_ms": round(float(np.percentile(a, 10)), 3),
                      "p90_ms": round(float(np.percentile(a, 90)), 3), "queries_per_s": round(B * 1e3 / med, 1),
                      "launches_per_call": launches[k]}
        res["speedup"] = round(res["per_query"]["median_ms"] / res["per_tile"]["median_ms"], 3)
        out["cases"][f"T{T}"] = res
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
