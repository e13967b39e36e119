"""numpy restatement of the position-prior forms (ccvpe_localize_prior, ccvpe_postprocess_prior, include/ccvpe.h), per query:

    l'         = fl32(logits + log_prior)          one float32 add per pixel
    m'         = max of l' (NaN ignored, as fmaxf)
    inv'       = 1 / sum exp(l' - m')              (float64 here; NaN when any l' is NaN or m' = +inf, inf when every l' is -inf)
    h'         = exp(l' - m') * inv'               the posterior heatmap (float64 here, __expf in float32 on the GPU)
    finite     = m' and inv' finite                otherwise the query has no posterior
    argmax row = (first argmax of h', h' there, ori at that pixel), or (-1, NaN, ...) without a posterior
    top-K rows = tests/topk_ref.topk_rows on h', or all (-1, 0, 0, 0, 0) without a posterior
"""
import numpy as np

from tests import topk_ref

N = 512 * 512


def posterior(logits, log_prior):
    """logits [B, n], log_prior [B, n] or [n] -> dict(h [B, n] float64, m [B], inv [B], finite [B] bool)."""
    lg = np.asarray(logits, np.float32).reshape(logits.shape[0], -1)
    lp = np.broadcast_to(np.asarray(log_prior, np.float32).reshape(-1, lg.shape[1]), lg.shape)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        l2 = (lg + lp).astype(np.float32).astype(np.float64)
        allnan = np.isnan(l2).all(axis=1)
        m = np.where(allnan, np.nan, np.nanmax(np.where(np.isnan(l2), -np.inf, l2), axis=1))
        e = np.exp(l2 - m[:, None])
        inv = 1.0 / e.sum(axis=1)
        finite = np.isfinite(m) & np.isfinite(inv)
        h = e * inv[:, None]
    return {"h": h, "m": m, "inv": inv, "finite": finite}


def argmax_rows(logits, ori, log_prior):
    """rows [B, 5] of the argmax form and margin [B] = relative gap between the best and the second-best h' (0 on a tie)."""
    post = posterior(logits, log_prior)
    h, fin = post["h"], post["finite"]
    B = h.shape[0]
    o = np.asarray(ori, np.float32).reshape(B, 2, -1)
    rows = np.zeros((B, 5), np.float32)
    margin = np.zeros(B)
    for b in range(B):
        if not fin[b]:
            rows[b, 0], rows[b, 1] = -1, np.nan
            continue
        i = int(np.argmax(h[b]))
        top2 = np.partition(h[b], -2)[-2:]
        margin[b] = (top2[1] - top2[0]) / top2[1]
        rows[b, :4] = (i, h[b, i], o[b, 0, i], o[b, 1, i])
        rows[b, 4] = topk_ref.angle_deg(rows[b, 2], rows[b, 3])
    return rows, margin


def topk_rows(logits, ori, log_prior, k, r):
    """rows [B, k, 5] of the top-K form on h' (rounded to float32), all (-1, 0, 0, 0, 0) for a query without a posterior."""
    post = posterior(logits, log_prior)
    B = post["h"].shape[0]
    side = int(round(np.sqrt(post["h"].shape[1])))
    heat = np.where(post["finite"][:, None], post["h"], 0.0).astype(np.float32).reshape(B, side, side)
    return topk_ref.topk_rows(heat, np.asarray(ori, np.float32).reshape(B, 2, side, side), k, r)
