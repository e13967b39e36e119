"""Per-launch times of the joint smoother (ccvpe_track_joint_smooth) against the time their compulsory bytes take at the
card's streaming rate.

    python tools/time_track_joint_smooth.py [--iters 5] [--warmup 2] [--window 20] [--repeats 5] [--out profiles/time_track_joint_smooth.json]

Cases: (nb, batch) in (8, 1), (36, 1), (36, 8), (72, 8); xy blur sigma 2 px, radius 6; heading blur radius 1; floor 1e-9; a fractional
shift per bin and a fractional turn; the sweep's in-place form (out=smoothed_next).  Both joints are synthetic (uniform random,
scaled to mass 1): no value changes what a launch moves.

The tool starts two fresh child processes, one after the other - tools/time_track_joint.py's protocol.  The first runs under
`rocprofv3 --kernel-trace` (the per-launch times are the dispatches' own durations): per case it issues a separator launch
(ccvpe_heading_predict), --warmup calls and --iters timed ones.  The second runs with no profiler attached and gives the whole-call
times: it first measures the streaming rate as tools/ubench_hbm.py does (a 1 GiB copy, read + write, and a 1 GiB read-only sum) on
the same card, then per case, after --warmup calls, times --window back-to-back calls between two device events, --repeats times,
and reports the median and the largest time per call.  The parent reads the trace, splits it at the separators and reports per
case and launch the median duration of the timed dispatches, the bytes the launch has to move (S = batch * nb maps of 1 MB):

    smooth.xy       2 S      the joint read, `work` written (the halo of a tile is re-read out of the cache)
    smooth.ratio    3 S      `work` (A) and the next joint read, h written over A
    smooth.weight   3 S      h and the joint read, w written
    smooth.scale    2 S + B  w read and scaled in place; the marginal written
    smooth.finish   -        partials only

and time-at-the-copy-rate / measured time.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((8, 1), (36, 1), (36, 8), (72, 8))
SIGMA, RADIUS, HTAPS, FLOOR, TURN = 2.0, 6, (0.8, 0.1), 1e-9, 7.3
MAP_BYTES = 4 * 512 * 512
SEPARATOR = "heading_predict_kernel"
LAUNCHES = {"track_joint_xy_kernel": "smooth.xy", "track_joint_smooth_ratio_kernel": "smooth.ratio",
            "track_joint_smooth_weight_kernel": "smooth.weight", "track_joint_smooth_scale_kernel": "smooth.scale",
            "track_joint_smooth_finish_kernel": "smooth.finish"}


def launch_bytes(batch: int, nb: int) -> dict:
    S = batch * nb
    return {"smooth.xy": 2 * S * MAP_BYTES, "smooth.ratio": 3 * S * MAP_BYTES, "smooth.weight": 3 * S * MAP_BYTES,
            "smooth.scale": (2 * S + batch) * MAP_BYTES, "smooth.finish": 0}


def worker(args) -> int:
    """one child: args.mode "trace" (under the profiler: the launches in a known order) or "calls" (no profiler: whole calls)"""
    import torch
    from ccvpe_amd import aerial, models, smooth, weights
    dev = torch.device("cuda", 0)
    traced = args.mode == "trace"

    def events(fn, n):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e-3

    prop = torch.cuda.get_device_properties(dev)
    out = {"device": {"name": torch.cuda.get_device_name(dev), "arch": getattr(prop, "gcnArchName", ""),
                      "compute_units": prop.multi_processor_count, "memory_GiB": round(prop.total_memory / 2 ** 30, 1),
                      "hip": torch.version.hip},
           "cases": {}}
    if not traced:
        # the streaming rates of tools/ubench_hbm.py, on this card, now
        n = (1 << 30) // 4
        x, y = torch.empty(n, device=dev), torch.empty(n, device=dev)
        x.fill_(1.0)
        copy_s = events(lambda: y.copy_(x), 10)
        sum_s = events(lambda: x.sum(), 10)
        del x, y
        torch.cuda.empty_cache()
        out["hbm_copy_TBps"] = round(2 * 1.0737e9 / copy_s / 1e12, 3)
        out["hbm_read_TBps"] = round(1.0737e9 / sum_s / 1e12, 3)
    model = models.CVM_OxfordRobotCar(dev)
    model.load_state_dict(weights.generate_state_dict("oxford", 0))
    model = model.to(dev).eval()
    taps = torch.as_tensor(aerial.gaussian_taps(SIGMA, RADIUS)).to(dev)
    htaps = torch.tensor(HTAPS, device=dev)
    sep_hist = torch.full((1, 8), 0.125, device=dev)
    for nb, batch in CASES:
        joint = torch.rand(batch, nb, 512, 512, device=dev)
        joint /= joint.sum(dim=(1, 2, 3), keepdim=True)
        run = torch.rand(batch, nb, 512, 512, device=dev)
        run /= run.sum(dim=(1, 2, 3), keepdim=True)
        shift = torch.as_tensor(aerial.joint_shift_table(np.full(batch, 9.37), np.full(batch, -0.6), nb), dtype=torch.float32).to(dev)
        turn, floor = torch.full((batch,), TURN, device=dev), torch.full((batch,), FLOOR, device=dev)

        def step():
            return smooth.track_joint_smooth(model, joint, run, shift, taps, floor, turn, htaps, out=run)

        case = {"nb": nb, "batch": batch, "joint_bytes": batch * nb * MAP_BYTES}
        if traced:
            model.heading_predict(sep_hist, 0.0, taps[:1] * 0 + 1.0, 0.0)        # the separator of the trace
            for _ in range(args.warmup + args.iters):
                step()
            torch.cuda.synchronize()
        else:
            for _ in range(args.warmup):
                step()
            ms = [events(step, args.window) * 1e3 for _ in range(args.repeats)]
            case["smooth_call_ms"] = round(float(np.median(ms)), 4)
            case["smooth_call_ms_max"] = round(float(max(ms)), 4)
        out["cases"][f"nb{nb}_b{batch}"] = case
        del joint, run
        torch.cuda.empty_cache()
    with open(args.worker, "w") as fh:
        json.dump(out, fh)
    return 0


def read_trace(trace_dir: str, warmup: int, iters: int) -> list:
    """the trace split at the separators: per segment {launch: [durations in us of the timed dispatches]}"""
    rows = []
    for f in glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    segments = []
    for r in rows:
        m = re.search("(" + "|".join([SEPARATOR] + list(LAUNCHES)) + ")", r["Kernel_Name"])
        if m and m.group(1) == SEPARATOR:
            segments.append({})
        elif m and segments:
            segments[-1].setdefault(LAUNCHES[m.group(1)], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for seg in segments:
        for k, v in seg.items():
            if len(v) != warmup + iters:
                raise SystemExit(f"{k}: {len(v)} dispatches in a segment of the trace, {warmup + iters} expected")
            seg[k] = v[warmup:]
    return segments


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--window", type=int, default=20, help="back-to-back calls per timed window of the untraced child")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per case and entry point")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--mode", default="calls", choices=["trace", "calls"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    with tempfile.TemporaryDirectory() as tmp:
        me = [sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--warmup", str(args.warmup), "--window", str(args.window),
              "--repeats", str(args.repeats)]
        results = {}
        for mode, front in (("trace", [prof, "--kernel-trace", "-d", os.path.join(tmp, "trace"), "-o", "run", "--output-format", "csv", "--"]),
                            ("calls", [])):
            res = os.path.join(tmp, mode + ".json")
            p = subprocess.run(front + me + ["--worker", res, "--mode", mode], cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                               text=True, timeout=900)
            if p.returncode != 0 or not os.path.exists(res):
                sys.stderr.write(p.stdout[-4000:])
                raise SystemExit(f"the {mode} child failed with status {p.returncode}")
            with open(res) as fh:
                results[mode] = json.load(fh)
        segments = read_trace(os.path.join(tmp, "trace"), args.warmup, args.iters)
    out = results["calls"]
    cases = list(out["cases"].values())
    if len(segments) != len(cases):
        raise SystemExit(f"{len(segments)} segments in the trace, {len(cases)} cases")
    rate = out["hbm_copy_TBps"] * 1e12
    for case, seg in zip(cases, segments):
        need = launch_bytes(case["batch"], case["nb"])
        case["launches"] = {}
        for name in LAUNCHES.values():
            us = float(np.median(seg[name]))
            row = {"median_us": round(us, 2), "max_us": round(float(max(seg[name])), 2), "bytes": need[name]}
            if need[name]:
                row["us_at_copy_rate"] = round(need[name] / rate * 1e6, 2)
                row["share_of_copy_rate"] = round(need[name] / rate * 1e6 / us, 3)
            case["launches"][name] = row
    out = {"tool": "tools/time_track_joint_smooth.py", "iters": args.iters, "warmup": args.warmup, "window": args.window, "repeats": args.repeats,
           "call_times": "no profiler attached: median and max over `repeats` windows of `window` back-to-back calls between device events",
           "launch_times": "rocprofv3 --kernel-trace of a second process: median and max of `iters` dispatches",
           "settings": {"sigma_px": SIGMA, "radius": RADIUS, "heading_taps": list(HTAPS), "floor": FLOOR, "turn_deg": TURN}, **out}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
