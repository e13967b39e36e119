"""The credible regions of a 512 x 512 map (include/ccvpe.h), restated in numpy by SORTING - not by the radix select
of kernels_credible.hip: a stable argsort of the keys, cumulative uint64 sums, and the first distinct key in descending order whose
cumulative mass reaches T.  Every number is an integer or one float64 operation on integers, so a device row is compared bit for bit."""
import numpy as np

HW = 512
N = HW * HW
SCALE = np.float32(2.0 ** 44)
LEVELS = (0.5, 0.9, 0.99, 1.0, 1e-6)


def keys_masses(h):
    """(uint32 keys, uint64 masses) of a map: the bit pattern and floorf(fminf(h, 1) * 2^44) where h > 0, else 0 (NaN compares false)"""
    f = np.ascontiguousarray(h, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        pos = f > 0
    k = np.where(pos, f.view(np.uint32), np.uint32(0)).astype(np.uint32)
    scaled = np.minimum(np.where(pos, f, np.float32(0)), np.float32(1)) * SCALE      # float32: exact (a power of two)
    q = np.floor(scaled).astype(np.uint64)
    return k, q


def threshold(p, Q):
    """T(p) of a total Q > 0: ceil((double)p * (double)Q), raised to 1, capped at Q"""
    t = np.ceil(np.float64(np.float32(p)) * np.float64(np.uint64(Q)))
    T = int(t)
    return min(max(T, 1), int(Q))


def credible(h, levels, probe=None, level_map=False):
    """(row float32 [4 + 3 L], uint8 map [512 * 512] or None) of one map; probe: a cell index or None"""
    k, q = keys_masses(h)
    L = len(levels)
    row = np.full(4 + 3 * L, np.nan, dtype=np.float32)
    Q = int(q.sum(dtype=np.uint64))
    row[0] = np.float32(np.float64(np.uint64(Q)) * 2.0 ** -44)
    row[1] = np.float32(int((k != 0).sum()))
    if probe is not None and 0 <= int(probe) < N:
        above_sel = k > k[int(probe)]
        above = int(q[above_sel].sum(dtype=np.uint64))
        row[3] = np.float32(int(above_sel.sum()))
        if Q > 0:
            row[2] = np.float32(np.float64(np.uint64(above)) / np.float64(np.uint64(Q)))
    lm = np.zeros(N, np.uint8) if level_map else None
    if Q == 0:
        for j in range(L):
            row[5 + 3 * j] = 0.0
        return row, lm
    order = np.argsort(k, kind="stable")[::-1]             # descending keys
    ks, qs = k[order], q[order]
    cum = np.cumsum(qs, dtype=np.uint64)
    last = np.flatnonzero(np.append(ks[1:] != ks[:-1], True))   # the last position of every distinct key: G and C of that key
    G = cum[last]
    for j, p in enumerate(levels):
        T = threshold(p, Q)
        i = int(np.searchsorted(G, np.uint64(T), side="left"))   # the first (largest) distinct key with G >= T
        kstar = ks[last[i]]
        assert kstar != 0
        row[4 + 3 * j] = np.array([kstar], np.uint32).view(np.float32)[0]
        row[5 + 3 * j] = np.float32(int(last[i]) + 1)
        row[6 + 3 * j] = np.float32(np.float64(G[i]) / np.float64(np.uint64(Q)))
        if lm is not None:
            lm += (k >= kstar).astype(np.uint8)
    return row, lm


def credibles(maps, levels, probes=None, level_map=False):
    """[B, 4 + 3 L] float32 (and [B, 512 * 512] uint8) of maps [B, 512, 512]"""
    maps = np.asarray(maps)
    out = [credible(m, levels, None if probes is None else probes[b], level_map) for b, m in enumerate(maps)]
    rows = np.stack([r for r, _ in out])
    return (rows, np.stack([m for _, m in out])) if level_map else rows


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
