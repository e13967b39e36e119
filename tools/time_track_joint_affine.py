"""Per-launch and whole-call times of the joint predict under an affine map per source heading bin (ccvpe_track_joint_predict_affine,
DESIGN.md 4.30) against ccvpe_track_joint_predict at the same sizes in the same session.

    python tools/time_track_joint_affine.py [--iters 5] [--warmup 2] [--window 50] [--repeats 5] [--out profiles/time_track_joint_affine.json]

Cases: nb in {8, 36, 72} x batch in {1, 8, 32} x four motions - `baseline`, ccvpe_track_joint_predict under a fractional shift per
bin; and ccvpe_track_joint_predict_affine under `translation` (the same shifts as matrices), `turn5` and `turn45` (the frame turned by
5 and by 45 degrees about its centre, the same shifts on top: aerial.joint_matrix_table).  xy blur sigma 2 px, radius 6; heading blur
radius 1; floor 1e-9; a fractional turn.  The joint is synthetic (uniform random): no value changes what a launch moves.

The tool starts two fresh child processes, one after the other.  The first runs under `rocprofv3 --kernel-trace` (the per-launch
times are the dispatches' own durations): per case it issues a separator launch (ccvpe_heading_predict), then --warmup calls and
--iters timed ones.  The second runs with no profiler attached and gives the whole-call times: per case, after --warmup calls, it
times --window back-to-back calls between two device events, --repeats times, and reports the median and the largest time per call.
The parent reads the trace, splits it at the separators and reports per case the median duration of the timed dispatches of the two
launches (xy or xy_affine, mix), the xy launch's time per map (batch * nb maps), and per size the ratios of the three affine
motions to the baseline - of the xy launch and of the whole call.  Prints one JSON line.
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

BINS, BATCHES = (8, 36, 72), (1, 8, 32)
MOTIONS = ("baseline", "translation", "turn5", "turn45")
TURNS = {"translation": 0.0, "turn5": 5.0, "turn45": 45.0}
SIGMA, RADIUS, HTAPS, FLOOR, TURN = 2.0, 6, (0.8, 0.1), 1e-9, 7.3
SEPARATOR = "heading_predict_kernel"
LAUNCHES = {"track_joint_xy_kernel": "xy", "track_joint_xy_affine_kernel": "xy_affine", "track_joint_mix_kernel": "mix"}


def worker(args) -> int:
    """one child: args.mode "trace" (under the profiler: the launches in a known order) or "calls" (no profiler: whole calls)"""
    import torch
    from ccvpe_amd import aerial, models, weights
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
    model = models.CVM_OxfordRobotCar(dev)
    model.load_state_dict(weights.generate_state_dict("oxford", 0))
    model = model.to(dev).eval()
    taps = torch.as_tensor(aerial.gaussian_taps(SIGMA, RADIUS)).to(dev)
    htaps = torch.tensor(HTAPS, device=dev)
    sep_hist = torch.full((1, 8), 0.125, device=dev)
    for nb in BINS:
        for batch in BATCHES:
            joint = torch.rand(batch, nb, 512, 512, device=dev)
            prior = torch.empty_like(joint)
            table = aerial.joint_shift_table(np.full(batch, 9.37), np.full(batch, -0.6), nb)
            shift = torch.as_tensor(table, dtype=torch.float32).to(dev)
            turn, floor = torch.full((batch,), TURN, device=dev), torch.full((batch,), FLOOR, device=dev)
            for motion in MOTIONS:
                if motion == "baseline":
                    def predict():
                        return model.track_joint_predict(joint, shift, taps, floor, turn, htaps, out=prior)
                else:
                    mats = torch.as_tensor(aerial.joint_matrix_table(aerial.rigid_matrix(TURNS[motion], (0.0, 0.0)), table)).to(dev)

                    def predict(mats=mats):
                        return model.track_joint_predict_affine(joint, mats, taps, floor, turn, htaps, out=prior)

                case = {"nb": nb, "batch": batch, "motion": motion}
                if traced:
                    model.heading_predict(sep_hist, 0.0, taps[:1] * 0 + 1.0, 0.0)        # the separator of the trace
                    for _ in range(args.warmup + args.iters):
                        predict()
                    torch.cuda.synchronize()
                else:
                    for _ in range(args.warmup):
                        predict()
                    ms = [events(predict, args.window) * 1e3 for _ in range(args.repeats)]
                    case["call_ms"] = round(float(np.median(ms)), 4)
                    case["call_ms_max"] = round(float(max(ms)), 4)
                out["cases"][f"nb{nb}_b{batch}_{motion}"] = case
            del joint, prior
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
    ap.add_argument("--window", type=int, default=50, help="back-to-back calls per timed window of the untraced child")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per case")
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
    for case, seg in zip(cases, segments):
        xy = "xy" if case["motion"] == "baseline" else "xy_affine"
        if sorted(seg) != sorted([xy, "mix"]):
            raise SystemExit(f"{case}: the trace holds the launches {sorted(seg)}")
        case["launches"] = {name: {"median_us": round(float(np.median(seg[name])), 2), "max_us": round(float(max(seg[name])), 2)}
                            for name in (xy, "mix")}
        case["xy_us_per_map"] = round(float(np.median(seg[xy])) / (case["batch"] * case["nb"]), 3)
    ratios = {}
    for nb in BINS:
        for batch in BATCHES:
            base = out["cases"][f"nb{nb}_b{batch}_baseline"]
            row = {}
            for motion in MOTIONS[1:]:
                c = out["cases"][f"nb{nb}_b{batch}_{motion}"]
                row[motion] = {"xy": round(c["launches"]["xy_affine"]["median_us"] / base["launches"]["xy"]["median_us"], 3),
                               "call": round(c["call_ms"] / base["call_ms"], 3)}
            ratios[f"nb{nb}_b{batch}"] = row
    out = {"tool": "tools/time_track_joint_affine.py", "iters": args.iters, "warmup": args.warmup, "window": args.window, "repeats": args.repeats,
           "call_times": "no profiler attached: median and max over `repeats` windows of `window` back-to-back calls between device events",
           "launch_times": "rocprofv3 --kernel-trace of a second process: median and max of `iters` dispatches",
           "ratios": "affine motion over the baseline (ccvpe_track_joint_predict) at the same size: the xy launch's median, the whole call's",
           "settings": {"sigma_px": SIGMA, "radius": RADIUS, "heading_taps": list(HTAPS), "floor": FLOOR, "turn_deg": TURN}, **out,
           "ratio_to_baseline": ratios}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
