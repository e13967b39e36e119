"""A/B of the plan builder refactor against the parent commit's library (profiles/refactor_plan_builder_ab.md):

    python tools/ab_plan_builder.py PARENT_LIB HEAD_LIB OUT_DIR

One Python package (this tree's), two libraries (CCVPE_LIB_PATH).  For each of four environments - the defaults, CCVPE_STREAMS=1,
CCVPE_FUSE_L1=0, CCVPE_COMPOSE_L6=1 - a fresh child process per library, parent then head, one after another, each under its own
`timeout`; the script stops at the first child that fails.  CCVPE_AUTOTUNE=0 and CCVPE_TUNE_CACHE=off in all of them: a tile the
shipped table does not hold comes from the shape heuristic, not from a measurement, so both libraries run the same launches.

A child runs the Oxford variant at 154x231 and the VIGOR variant at 320x640, batches 1 and 3: every form family (forward, localize,
top-K, prior, track update, summary, heading, heading prior, credible) on the image pair, on an aerial cache (plain and indexed) and
through localize_region, plus the two encode calls, with seeded inputs.  After each call it records the SHA-256 of every result tensor,
the ccvpe_launch_count delta and the text of ccvpe_debug_dump_plan (names, streams, waits, tile names, offsets, sizes and the integer
checksum of every plan tensor); at the end the ccvpe_export_tuning text of each model, whose keys hold the GEMM shape and the eligibility
flags of every tiled launch of every plan built.  The parent writes OUT_DIR/ab_plan_builder.md: per environment and call, tensors
that differ, launch counts, dump lines that differ, and the tuning key sets.

With CCVPE_AUTOTUNE=0 nothing is recorded, so that export is the shipped table on both sides and the keys of the plans built show only
where the table holds them (the batch-1 plans: a launch whose key changed would lose its tile name in the dump).  A fourth argument
`keys` runs one more pair of children with the autotuner on, batch 3 only, and compares the exported KEY SETS alone: the tiles
then come from measurements and may differ, the keys - launch name, GEMM shape, eligibility flags, with real packed weights - may not."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS = [("defaults", {}), ("CCVPE_STREAMS=1", {"CCVPE_STREAMS": "1"}), ("CCVPE_FUSE_L1=0", {"CCVPE_FUSE_L1": "0"}),
        ("CCVPE_COMPOSE_L6=1", {"CCVPE_COMPOSE_L6": "1"})]
KEYS_ENV = ("autotune on, batch 3: tuning key sets only", {"AB_KEYS_ONLY": "1"})
CHILD_TIMEOUT_S = 420


def child(out_path):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from ccvpe_amd import _lib, aerial, models, weights

    lib = _lib.load()
    N = 512 * 512
    calls = []

    def flat(res):
        if isinstance(res, dict):
            return [res[k] for k in sorted(res)]
        return list(res) if isinstance(res, (tuple, list)) else [res]

    def sha(t):
        a = t if isinstance(t, np.ndarray) else t.detach().contiguous().cpu().numpy()
        return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

    def run(m, name, fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        res = fn()
        torch.cuda.synchronize()
        launches = int(lib.ccvpe_launch_count() - n0)
        path = out_path + ".dump"
        _lib.check(lib.ccvpe_debug_dump_plan(m._handle, path.encode()), "ccvpe_debug_dump_plan")
        calls.append({"name": name, "tensors": [sha(t) for t in flat(res) if isinstance(t, (torch.Tensor, np.ndarray))], "launches": launches,
                      "dump": open(path).read().splitlines()})
        os.remove(path)
        return res

    tuning = {}
    for variant, make in (("oxford", lambda: models.CVM_OxfordRobotCar("cuda")), ("vigor", lambda: models.CVM_VIGOR("cuda", True))):
        m = make()
        m.load_state_dict(weights.generate_state_dict(variant, 0))
        m = m.to("cuda").eval()
        for B in ((3,) if os.environ.get("AB_KEYS_ONLY") else (1, 3)):
            g, s = weights.generate_inputs(variant, B, 11, 360.0)
            g, s = torch.from_numpy(g).cuda(), torch.from_numpy(s).cuda()
            rng = np.random.default_rng(5)
            lp = aerial.gaussian_log_prior(rng.uniform(60, 452, size=(B, 2)), 40.0, "cuda")
            tb = torch.from_numpy(aerial.von_mises_heading_log_prior([10.0, 140.0, 300.0][:B], 3.0, 72)).cuda()
            levels, probe = (0.5, 0.9, 0.99), [5, 512 * 200 + 17, N - 1][:B]
            idx = [2, 0, 1][:B] if B == 3 else [0]
            tag = f"{variant}@b{B} "
            run(m, tag + "forward", lambda: m(g, s))      # first: the dump is of the last forward-family plan, the encode calls leave it
            sc = run(m, tag + "encode_aerial", lambda: m.encode_aerial(s))
            gc = run(m, tag + "encode_ground", lambda: m.encode_ground(g))
            sides = [("", lambda f, *a, **k: getattr(m, f)(g, s, *a, **k)),
                     ("_cached", lambda f, *a, **k: getattr(m, f + "_cached")(g, sc, *a, **k)),
                     ("_cached_idx", lambda f, *a, **k: getattr(m, f + "_cached")(g, sc, *a, tile_index=idx, **k))]
            for side, call in sides:
                if side != "":
                    run(m, tag + "forward" + side, lambda: m.forward_cached(g, sc, idx if side == "_cached_idx" else None))
                run(m, tag + "localize" + side, lambda: call("localize"))
                run(m, tag + "localize_topk" + side, lambda: call("localize_topk", 8, 8))
                run(m, tag + "localize_prior_k0" + side, lambda: call("localize_prior", lp))
                run(m, tag + "localize_prior_k4" + side, lambda: call("localize_prior", lp, 4, 8))
                run(m, tag + "track_update" + side, lambda: call("track_update", lp))
                run(m, tag + "localize_summary" + side, lambda: call("localize_summary", lp, radius=8, posterior=True))
                run(m, tag + "localize_heading" + side, lambda: call("localize_heading", lp, radius=8, bins=36, posterior=True))
                run(m, tag + "localize_heading_summary" + side, lambda: call("localize_heading", None, bins=72, summary=True))
                run(m, tag + "localize_heading_prior" + side, lambda: call("localize_heading_prior", tb, lp, radius=8, bins=36, summary=True, posterior=True))
                run(m, tag + "localize_credible" + side, lambda: call("localize_credible", levels, lp, probe, level_map=True, posterior=True))
            tiles = [[0, 1], [2], [1, 0, 2]] if B == 3 else [[0]]
            npairs = sum(len(t) for t in tiles)
            run(m, tag + "localize_region", lambda: m.localize_region(gc, sc, tiles))
            plp = aerial.gaussian_log_prior(rng.uniform(60, 452, size=(npairs, 2)), 50.0, "cuda")
            run(m, tag + "localize_region_prior", lambda: m.localize_region_prior(gc, sc, tiles, plp))
        tuning[variant] = m.export_tuning().splitlines()
        del m
        torch.cuda.empty_cache()
    json.dump({"calls": calls, "tuning": tuning}, open(out_path, "w"))
    print("child", os.environ.get("CCVPE_LIB_PATH"), len(calls), "calls", sum(len(c["tensors"]) for c in calls), "tensors", flush=True)


def tuning_keys(lines):
    return sorted(" ".join(ln.split()[:2]) for ln in lines if ln.startswith("op "))


def main():
    if sys.argv[1] == "child":
        return child(sys.argv[2])
    libs = {"parent": os.path.abspath(sys.argv[1]), "head": os.path.abspath(sys.argv[2])}
    out_dir = sys.argv[3]
    os.makedirs(out_dir, exist_ok=True)
    md = ["| environment | call | result tensors (differing) | launches parent / head | dump lines (differing) |", "|---|---|---|---|---|"]
    totals = {"calls": 0, "tensors": 0, "tensors_diff": 0, "launch_diff": 0, "lines": 0, "lines_diff": 0}
    tune_md = []
    keys_only = len(sys.argv) > 4 and sys.argv[4] == "keys"
    for env_name, extra in ([KEYS_ENV] if keys_only else ENVS):
        res = {}
        for tag, lib in libs.items():
            env = {k: v for k, v in os.environ.items() if not k.startswith("CCVPE_")}
            env.update(extra, CCVPE_LIB_PATH=lib, CCVPE_TUNE_CACHE="off")
            if not keys_only:
                env["CCVPE_AUTOTUNE"] = "0"
            path = os.path.join(out_dir, "child_%s.json" % tag)
            r = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "child", path], env=env)
            if r.returncode != 0:
                print("child failed:", env_name, tag, "exit", r.returncode, flush=True)
                return r.returncode
            res[tag] = json.load(open(path))
            os.remove(path)
        p, h = res["parent"], res["head"]
        assert [c["name"] for c in p["calls"]] == [c["name"] for c in h["calls"]]
        for a, b in zip(p["calls"], [] if keys_only else h["calls"]):
            td = sum(x != y for x, y in zip(a["tensors"], b["tensors"])) + abs(len(a["tensors"]) - len(b["tensors"]))
            ld = sum(x != y for x, y in zip(a["dump"], b["dump"])) + abs(len(a["dump"]) - len(b["dump"]))
            md.append("| %s | `%s` | %d (%d) | %d / %d | %d (%d) |" % (env_name, a["name"], len(a["tensors"]), td, a["launches"], b["launches"], len(a["dump"]), ld))
            totals["calls"] += 1; totals["tensors"] += len(a["tensors"]); totals["tensors_diff"] += td
            totals["launch_diff"] += a["launches"] != b["launches"]; totals["lines"] += len(a["dump"]); totals["lines_diff"] += ld
        for variant in p["tuning"]:
            kp, kh = tuning_keys(p["tuning"][variant]), tuning_keys(h["tuning"][variant])
            same_text = p["tuning"][variant] == h["tuning"][variant]
            tune_md.append("| %s | %s | %d | %d | %s | %s |" % (env_name, variant, len(kp), len(kh), "identical" if kp == kh else "DIFFERENT",
                                                              "identical" if same_text else "DIFFERENT"))
            totals["lines_diff"] += 0 if kp == kh else 1
        print(env_name, totals, flush=True)
    text = ["%(calls)d calls: %(tensors)d result tensors, %(tensors_diff)d differ; %(launch_diff)d launch counts differ; %(lines)d dump lines, "
            "%(lines_diff)d differ (tuning key sets included)" % totals, ""] + md
    text += ["", "| environment | model | tuning keys parent | head | key sets | export text |", "|---|---|---|---|---|---|"] + tune_md
    open(os.path.join(out_dir, "ab_plan_builder_keys.md" if keys_only else "ab_plan_builder.md"), "w").write("\n".join(text) + "\n")
    print(text[0], flush=True)
    return 0 if totals["tensors_diff"] == 0 and totals["launch_diff"] == 0 and totals["lines_diff"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
