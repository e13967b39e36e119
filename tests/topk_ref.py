"""numpy restatement of the top-K peak definition of ccvpe_postprocess_topk / ccvpe_localize_topk (include/ccvpe.h).

For one map H (float32 [h, w], flat index p = y * w + x), a radius r and a count k:
  - q suppresses p when q != p, max(|qy - py|, |qx - px|) <= r (clipped at the border) and H[q] > H[p], or H[q] == H[p] and
    q < p.  A NaN neighbour never suppresses.
  - p is a peak when H[p] > 0 and nothing suppresses it.
  - peaks are ordered by value (descending), then index (ascending); the first k are kept.

The two parts of "suppresses" are written separately:
  - the tie-break is an order on pixels, `order_key`: one integer per pixel that is larger exactly when the pixel wins;
  - the window comparison, `window_max`: the largest key over every pixel's Chebyshev window.
p is a peak iff its key is positive and it equals the window maximum.
"""
import numpy as np

INDEX_BITS = 20   # indices below 2^20 (512 x 512 maps and the small test maps)


def order_key(H):
    """int64 key per pixel: (value, -index) in lexicographic order for H > 0; 0 for zeros, negatives and NaN, which never
    suppress anything and are never peaks.  Positive float32 values order like their bit patterns."""
    H = np.ascontiguousarray(H, dtype=np.float32)
    n = H.size
    assert n <= 1 << INDEX_BITS
    bits = H.view(np.uint32).astype(np.int64)
    inv_index = (1 << INDEX_BITS) - 1 - np.arange(n, dtype=np.int64).reshape(H.shape)
    with np.errstate(invalid="ignore"):
        positive = H > 0
    return np.where(positive, (bits << INDEX_BITS) | inv_index, 0)


def _sliding_max_1d(a, r, axis):
    """max over [i - r, i + r] along `axis`, positions outside the array ignored (padded with 0, the smallest key)."""
    if r == 0:
        return a.copy()
    n = a.shape[axis]
    pad = [(0, 0)] * a.ndim
    pad[axis] = (r, r)
    p = np.pad(a, pad)
    out = np.take(p, np.arange(0, n), axis=axis)
    for d in range(1, 2 * r + 1):
        out = np.maximum(out, np.take(p, np.arange(d, d + n), axis=axis))
    return out


def window_max(key, r):
    """The largest key over each pixel's (2r + 1)^2 Chebyshev window, clipped at the border (separable)."""
    return _sliding_max_1d(_sliding_max_1d(key, r, 1), r, 0)


def peaks(H, r):
    """Boolean map of the peaks of H under radius r."""
    key = order_key(H)
    return (key > 0) & (window_max(key, r) == key)


def peak_indices(H, r, k):
    """Flat indices of the first k peaks in (value desc, index asc) order."""
    key = order_key(H)
    mask = (key > 0) & (window_max(key, r) == key)
    sel = key[mask]
    order = np.argsort(-sel, kind="stable")[:k]
    return ((1 << INDEX_BITS) - 1 - (sel[order] & ((1 << INDEX_BITS) - 1))).astype(np.int64)


def angle_deg(cs, sn):
    """pose_angle_deg of the post-processing kernels in float32 (train_VIGOR.py:307-311)."""
    cs = np.asarray(cs, np.float32)
    sn = np.asarray(sn, np.float32)
    ang = (np.arccos(np.clip(cs, np.float32(-1), np.float32(1))) * np.float32(57.29577951308232)).astype(np.float32)
    neg = np.fmod(-ang, np.float32(360)).astype(np.float32)
    neg = np.where(neg < 0, neg + np.float32(360), neg).astype(np.float32)
    return np.where(sn < 0, neg, ang).astype(np.float32)


def topk_rows(heat, ori, k, r, angle=angle_deg):
    """rows [B, k, 5] = (index, prob, cos, sin, angle_deg) for heat [B, h, w] and ori [B, 2, h, w]; (-1, 0, 0, 0, 0) past the
    last peak.  `angle` maps (cos, sin) arrays to the angle column."""
    heat = np.asarray(heat, np.float32)
    ori = np.asarray(ori, np.float32)
    B = heat.shape[0]
    rows = np.zeros((B, k, 5), np.float32)
    rows[:, :, 0] = -1
    for b in range(B):
        idx = peak_indices(heat[b], r, k)
        n = len(idx)
        flat_h = heat[b].reshape(-1)
        flat_o = ori[b].reshape(2, -1)
        rows[b, :n, 0] = idx.astype(np.float32)
        rows[b, :n, 1] = flat_h[idx]
        rows[b, :n, 2] = flat_o[0, idx]
        rows[b, :n, 3] = flat_o[1, idx]
    valid = rows[:, :, 0] >= 0
    ang = np.asarray(angle(rows[:, :, 2], rows[:, :, 3]), np.float32)
    rows[:, :, 4] = np.where(valid, ang, np.float32(0))
    return rows
