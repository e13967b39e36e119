"""numpy restatement of ccvpe_localize_region's cross-tile reduction (region_reduce_kernel), in float64:

    m_p, inv_p = stats[p]                          (pose_argmax_kernel's softmax max and 1 / sum of pair p's tile)
    M          = max of m_p over the query's pairs with finite (m_p, inv_p)
    S_p        = exp(m_p - M) / inv_p              (0 for a pair whose statistics are not finite)
    Z          = sum_p S_p
    tile_prob  = float32(S_p / Z)
    joint_p    = float64(prob_p) * S_p / Z         (the joint softmax over all the query's pixels at pair p's argmax)
    best       = first finite pair with the largest joint_p (NaN never wins); none: the query's first pair, prob NaN
    rows[g]    = (index, float32(joint_best), cos, sin, angle) of pair_rows[best]
"""
import numpy as np


def region_reduce(offsets, stats, pair_rows):
    """offsets [G+1], stats [P,2] float32, pair_rows [P,5] float32 -> dict(rows [G,5] f32, best_pair [G] int, tile_prob [P] f32,
    joint [P] f64, margin [G] f64 = relative gap between the best and the runner-up joint probability, inf without a runner-up)"""
    off = np.asarray(offsets, dtype=np.int64)
    st = np.asarray(stats, dtype=np.float32).reshape(-1, 2)
    pr = np.asarray(pair_rows, dtype=np.float32).reshape(-1, 5)
    G = off.shape[0] - 1
    rows = np.empty((G, 5), dtype=np.float32)
    best_pair = np.empty(G, dtype=np.int64)
    tile_prob = np.empty(st.shape[0], dtype=np.float32)
    joint = np.full(st.shape[0], np.nan)
    margin = np.full(G, np.inf)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for g in range(G):
            lo, hi = int(off[g]), int(off[g + 1])
            m = st[lo:hi, 0].astype(np.float64)
            inv = st[lo:hi, 1].astype(np.float64)
            fin = np.isfinite(m) & np.isfinite(inv)
            M = m[fin].max() if fin.any() else -np.inf
            S = np.where(fin, np.exp(np.where(fin, m, 0.0) - M) / np.where(fin, inv, 1.0), 0.0)
            Z = S.sum()
            tile_prob[lo:hi] = (S / Z).astype(np.float32)
            j = pr[lo:hi, 1].astype(np.float64) * S / Z
            joint[lo:hi] = j
            ok = fin & ~np.isnan(j)
            if ok.any():
                cand = np.where(ok, j, -np.inf)
                b = int(np.argmax(cand))          # first maximal position
                prob = np.float32(j[b])
                # pairs with the best pair's very statistics and probability (a repeated tile) tie exactly in any evaluation order,
                # and the first wins: they do not count as runners-up
                same = (st[lo:hi, 0] == st[lo + b, 0]) & (st[lo:hi, 1] == st[lo + b, 1]) & (pr[lo:hi, 1] == pr[lo + b, 1])
                rest = cand[~same]
                if rest.size and np.isfinite(rest).any():
                    margin[g] = (j[b] - rest.max()) / max(abs(j[b]), 1e-300)
            else:
                b, prob = 0, np.float32(np.nan)
            best_pair[g] = lo + b
            rows[g] = pr[lo + b]
            rows[g, 1] = prob
    return {"rows": rows, "best_pair": best_pair, "tile_prob": tile_prob, "joint": joint, "margin": margin}


def query_of_pair(offsets):
    off = np.asarray(offsets, dtype=np.int64)
    return np.repeat(np.arange(off.shape[0] - 1), np.diff(off))
