"""One child process of the Python front end A/B (profiles/refactor_python_front_ab.md):

    CCVPE_LIB_PATH=<built libccvpe_hip.so> CCVPE_AUTOTUNE=0 CCVPE_TUNE_CACHE=off python tools/ab_python_front.py DIR TAG OUT.json [speed]

DIR holds the ccvpe_amd package to import: the tree, or a directory with another commit's ccvpe_amd/*.py and ccvpe_amd/tuning/.  Both
packages load the one library CCVPE_LIB_PATH names.  Writes the SHA-256 of every output tensor of the call list (skipped with a
fourth argument) and calls per second of four batch-1 calls, two windows of about 1.2 s each that end in a synchronise.  Run the
children alternately - parent, head, parent, head ... - and compare: equal hashes, and the head's median window of a case inside the
range of the parent's windows."""
import hashlib
import json
import sys
import time

sys.path.insert(0, sys.argv[1])
import numpy as np
import torch

import ccvpe_amd
from ccvpe_amd import aerial, models, weights

assert ccvpe_amd.__file__.startswith(sys.argv[1]), (ccvpe_amd.__file__, sys.argv[1])
N = 512 * 512


def sha(t):
    if isinstance(t, np.ndarray):
        return hashlib.sha256(np.ascontiguousarray(t).tobytes()).hexdigest()
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def flat(res):
    if isinstance(res, dict):
        return [res[k] for k in sorted(res)]
    return list(res) if isinstance(res, (tuple, list)) else [res]


def main():
    torch.manual_seed(0)
    m = models.CVM_VIGOR_ori_prior("cuda", 180.0, True)
    m.load_state_dict(weights.generate_state_dict("vigor_ori_prior", 0))
    m = m.to("cuda").eval()
    B = 3
    g, s = weights.generate_inputs("vigor_ori_prior", B, 11, 360.0)
    g, s = torch.from_numpy(g).cuda(), torch.from_numpy(s).cuda()
    rng = np.random.default_rng(5)
    lp = aerial.gaussian_log_prior(rng.uniform(60, 452, size=(B, 2)), 40.0, "cuda")
    lp1 = aerial.gaussian_log_prior(rng.uniform(60, 452, size=(1, 2)), 80.0, "cuda")[0]
    tbB = torch.from_numpy(aerial.von_mises_heading_log_prior([10.0, 140.0, 300.0], 3.0, 72)).cuda()
    tb1 = torch.from_numpy(aerial.von_mises_heading_log_prior(77.0, 1.0, 20)).cuda()
    levels, probe = (0.5, 0.9, 0.99), [5, 512 * 200 + 17, N - 1]
    out = {}

    def rec(name, res):
        assert name not in out, name
        out[name] = [sha(t) for t in flat(res)]

    fwd = m(g, s)
    good = fwd[1].view(B, 512, 512).contiguous()
    if len(sys.argv) <= 4:      # a fourth argument: speed only
        rec("forward", fwd)
        sc = m.encode_aerial(s)
        idx = [2, 0, 1]
        rec("forward_cached", m.forward_cached(g, sc))
        rec("forward_cached_idx", m.forward_cached(g, sc, idx))
        rec("localize", m.localize(g, s))
        rec("localize_cached", m.localize_cached(g, sc))
        rec("localize_cached_idx", m.localize_cached(g, sc, idx))
        rec("localize_topk", m.localize_topk(g, s, 8, 8))
        rec("localize_topk_cached_idx", m.localize_topk_cached(g, sc, 8, 8, idx))
        rec("localize_prior_k0", m.localize_prior(g, s, lp))
        rec("localize_prior_k4", m.localize_prior(g, s, lp, 4, 8))
        rec("localize_prior_cached_k4", m.localize_prior_cached(g, sc, lp1, 4, 8, tile_index=idx))
        rec("track_update", m.track_update(g, s))
        rec("track_update_prior", m.track_update(g, s, lp))
        rec("track_update_cached", m.track_update_cached(g, sc, lp, tile_index=idx))
        rec("localize_summary", m.localize_summary(g, s, lp, radius=8, posterior=True))
        rec("localize_summary_bare", m.localize_summary(g, s))
        rec("localize_summary_cached", m.localize_summary_cached(g, sc, lp, radius=4, posterior=True, tile_index=idx))
        rec("localize_heading_full", m.localize_heading(g, s, lp, radius=8, bins=36, summary=True, posterior=True))
        rec("localize_heading_bare", m.localize_heading(g, s, bins=36))
        rec("localize_heading_cached", m.localize_heading_cached(g, sc, lp, bins=72, summary=True, tile_index=idx))
        rec("localize_heading_prior_full", m.localize_heading_prior(g, s, tbB, lp, radius=8, bins=36, summary=True, posterior=True))
        rec("localize_heading_prior_one", m.localize_heading_prior(g, s, tb1))
        rec("localize_heading_prior_cached", m.localize_heading_prior_cached(g, sc, tbB, lp, bins=36, posterior=True, tile_index=idx))
        rec("localize_credible_full", m.localize_credible(g, s, levels, lp, probe, level_map=True, posterior=True))
        rec("localize_credible_bare", m.localize_credible(g, s, levels))
        rec("localize_credible_cached", m.localize_credible_cached(g, sc, levels, lp, probe, level_map=True, tile_index=idx))
        gc = m.encode_ground(g)
        tiles = [[0, 1], [2], [1, 0, 2]]
        rec("localize_region", m.localize_region(gc, sc, tiles))
        plp = aerial.gaussian_log_prior(rng.uniform(60, 452, size=(6, 2)), 50.0, "cuda")
        rec("localize_region_prior", m.localize_region_prior(gc, sc, tiles, plp))
        # held and stored forms on the forward's outputs: sample 1 all NaN, sample 2 quantised so that thousands of cells tie
        lg, heat, ori = (t.clone() for t in fwd[:3])
        lg[1] = float("nan")
        heat[1] = float("nan")
        lg[2] = torch.round(lg[2] * 4.0) / 4.0
        heat[2] = torch.softmax(lg[2], dim=0).view(1, 512, 512)
        top = torch.topk(heat[2].view(-1), 10).indices
        heat[2].view(-1)[top] = heat[2].max()
        rec("postprocess", m.postprocess(heat, ori))
        rec("postprocess_rows", m.postprocess_rows(heat, ori))
        rec("postprocess_topk", m.postprocess_topk(heat, ori, 8, 8))
        rec("postprocess_prior_k0", m.postprocess_prior(lg, ori, lp))
        rec("postprocess_prior_k4", m.postprocess_prior(lg, ori, lp, 4, 8))
        rec("track_update_logits", m.track_update_logits(lg, ori))
        rec("track_update_logits_prior", m.track_update_logits(lg, ori, lp))
        rec("postprocess_summary", m.postprocess_summary(lg, ori, lp, radius=8, posterior=True))
        rec("postprocess_summary_r32", m.postprocess_summary(lg, ori, radius=32))
        rec("postprocess_heading", m.postprocess_heading(lg, ori, lp, radius=8, bins=36, summary=True, posterior=True))
        rec("postprocess_heading_r32", m.postprocess_heading(lg, ori, radius=32, bins=72))
        rec("postprocess_credible", m.postprocess_credible(lg, ori, levels, lp, probe, level_map=True, posterior=True))
        rec("postprocess_credible_bare", m.postprocess_credible(lg, ori, levels))
        rec("heading_prior_map", m.heading_prior_map(ori, tbB, lp))
        rec("heading_prior_map_one", m.heading_prior_map(ori, tb1))
        bel = heat.view(B, 512, 512).contiguous()
        rec("belief_summary", m.belief_summary(bel, 8))
        odd = torch.zeros(B * N + 1, device="cuda")[1:].view(B, 512, 512)
        odd.copy_(fwd[1].view(B, 512, 512))
        rec("belief_summary_r32_unaligned", m.belief_summary(odd, 32))
        rec("belief_credible", m.belief_credible(bel, levels, probe, level_map=True))
        rec("belief_credible_bare", m.belief_credible(fwd[1], levels))
        good = fwd[1].view(B, 512, 512).contiguous()
        shifts = rng.uniform(-40, 40, size=(B, 2))
        for r in (0, 6, 32):
            taps = aerial.gaussian_taps(max(r / 3.0, 0.5), r)
            rec(f"track_predict_r{r}", m.track_predict(good, shifts, taps, 1e-7))
            mat = aerial.rigid_matrix([7.0, -31.0, 0.0], shifts, [1.0, 1.1, 1.0])
            rec(f"track_predict_affine_r{r}", m.track_predict_affine(good, mat, taps, np.full(B, 1e-7)))
        hist = m.localize_heading(g, s, bins=72)[2]
        rec("heading_predict", m.heading_predict(hist, [3.0, -50.5, 181.0], aerial.gaussian_taps(2.0, 6), 1e-3))
        rec("heading_predict_shared", m.heading_predict(hist, 12.5, aerial.gaussian_taps(1.0, 3)[None].repeat(B, 0), np.full(B, 1e-4)))
        # the trackers, two frames
        tr, at = aerial.Tracker(), aerial.AffineTracker()
        hk = dict(heading_bins=36, heading_turn_deg=5.0, heading_taps=aerial.gaussian_taps(2.0, 6), heading_floor=1e-3)
        org = np.array([[800, 400], [1200, 400], [800, 800]])
        for k in range(2):
            gk = torch.roll(g, 13 * k, dims=3)
            rec(f"tracker_{k}", tr.step(m, gk, sc, idx, org, [30.0, -7.5], aerial.gaussian_taps(3.0, 9), 1e-7, summary_radius=8, credible_levels=levels, **hk))
            rec(f"affine_tracker_{k}", at.step(m, gk, s, aerial.rigid_matrix(3.0, [4.5, -2.0]), aerial.gaussian_taps(3.0, 9), 1e-7, summary_radius=4, **hk))
    torch.cuda.synchronize()

    # ---- speed: calls per second at batch 1 ------------------------------------------------------------------------------------------
    g1, s1 = g[:1].contiguous(), s[:1].contiguous()
    sc1 = m.encode_aerial(s1)
    lp_1 = lp[:1].contiguous()
    b1 = good[:1].contiguous()
    sh1, taps6 = torch.tensor([[3.5, -2.25]], device="cuda"), torch.from_numpy(aerial.gaussian_taps(2.0, 6)).cuda()
    cases = {
        "localize_b1": lambda: m.localize(g1, s1),
        "localize_heading_cached_b1": lambda: m.localize_heading_cached(g1, sc1, lp_1, radius=8, bins=72, summary=True, posterior=True),
        "belief_summary_b1": lambda: m.belief_summary(b1, 8),
        "track_predict_r6_b1": lambda: m.track_predict(b1, sh1, taps6, 1e-7),
    }
    speed = {}
    for name, fn in cases.items():
        for _ in range(50):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        while time.perf_counter() - t0 < 0.3:       # size a window of about 1.2 s
            fn()
            n += 1
        torch.cuda.synchronize()
        reps = max(50, int(n * 1.2 / (time.perf_counter() - t0)))
        speed[name] = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            speed[name].append(reps / (time.perf_counter() - t0))
    json.dump({"tag": sys.argv[2], "package": ccvpe_amd.__file__, "hashes": out, "calls_per_s": speed}, open(sys.argv[3], "w"), indent=1)
    print(sys.argv[2], "tensors", sum(len(v) for v in out.values()), "calls", len(out), {k: [round(x, 1) for x in v] for k, v in speed.items()})


main()
