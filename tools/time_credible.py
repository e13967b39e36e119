"""Credible regions of stored maps (ccvpe_belief_credible) against ccvpe_belief_summary on the same maps, in one process.

    python tools/time_credible.py [--rounds 20] [--calls 10] [--warmup 5] [--out profiles/time_credible.json]

Maps: the posterior of a network forward (vigor_samearea_fov360_b32 built as bench.py builds it, weights.generate_state_dict(variant, 0),
weights.generate_inputs; track_update's map) and the uniform map, the case in which every cell of every pass shares one bucket.  Batch 1
(the tracker's case: the first map) and batch 32.  Forms: belief_summary (one read of the map, the yardstick), belief_credible with
three levels (0.5, 0.9, 0.99) without and with the level map (four and five launches, as many reads).

Every form is warmed up; then the forms alternate over --rounds rounds (the order rotates), each round --calls back-to-back calls between
two hipEvents on the current stream.  Prints one JSON line: per case and form the median, smallest and largest time per call in
microseconds and the library's launches per call, and per case credible / summary - to be read against the ratio of reads, 4 and 5.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVELS = (0.5, 0.9, 0.99)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    from ccvpe_amd import _lib, models, weights
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    m = models.CVM_VIGOR_ori_prior(dev, 180.0, True)
    m.load_state_dict(weights.generate_state_dict("vigor_ori_prior", 0))
    m = m.to(dev).eval()
    g, s = weights.generate_inputs("vigor_ori_prior", 32, 0, 360.0)
    network = m.track_update(torch.from_numpy(g).to(dev), torch.from_numpy(s).to(dev))[1].contiguous()
    uniform = torch.full((32, 512, 512), 1.0 / (512 * 512), dtype=torch.float32, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.calls, int(lib.ccvpe_launch_count() - n0) // args.calls

    out = {"tool": "tools/time_credible.py", "rounds": args.rounds, "calls_per_round": args.calls, "levels": list(LEVELS),
           "device": torch.cuda.get_device_name(dev), "cases": {}}
    for mname, maps in (("network", network), ("uniform", uniform)):
        for batch in (1, 32):
            bel = maps[:batch].contiguous()
            # the C entry points on preallocated results: no allocation and no argument checking of the Python layer between the events
            summ = torch.empty((batch, 16), dtype=torch.float32, device=dev)
            cred = torch.empty((batch, 4 + 3 * len(LEVELS)), dtype=torch.float32, device=dev)
            lmap = torch.empty((batch, 512, 512), dtype=torch.uint8, device=dev)
            lv = (C.c_float * len(LEVELS))(*LEVELS)
            h, st = m._handle, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            bp, sp, cp, lp = (C.c_void_p(t.data_ptr()) for t in (bel, summ, cred, lmap))

            def call(rc):
                if rc != 0:
                    raise RuntimeError(lib.ccvpe_last_error().decode())

            forms = {"summary": lambda: call(lib.ccvpe_belief_summary(h, bp, batch, 8, sp, st)),
                     "credible": lambda: call(lib.ccvpe_belief_credible(h, bp, batch, lv, len(LEVELS), None, cp, None, st)),
                     "credible_level_map": lambda: call(lib.ccvpe_belief_credible(h, bp, batch, lv, len(LEVELS), None, cp, lp, st))}
            for _ in range(args.warmup):
                for fn in forms.values():
                    fn()
            names = list(forms)
            us = {n: [] for n in names}
            launches = {}
            for i in range(args.rounds):
                k = i % len(names)
                for n in names[k:] + names[:k]:
                    t, c = timed(forms[n])
                    us[n].append(t)
                    launches[n] = c
            res = {}
            for n in names:
                a = np.asarray(us[n])
                res[n] = {"median_us": round(float(np.median(a)), 2), "min_us": round(float(a.min()), 2), "max_us": round(float(a.max()), 2),
                          "library_launches_per_call": launches[n]}
            for n in names[1:]:
                res[n + "_over_summary"] = round(res[n]["median_us"] / res["summary"]["median_us"], 2)
            out["cases"][f"{mname}_b{batch}"] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
