"""numpy restatement of the heading prior (include/ccvpe.h) on top of tests/heading_ref.Field.

The combined prior map of a table T [nb + 1] (float32 log-weights; entry nb for a cell without a heading) and an optional position
prior P, per cell i:

    k_i = valid(c_i, s_i) ? bin_nb(c_i, s_i) : nb        comb_i = T[k_i]   or   fl32(P_i + T[k_i])

in float32 from the Field's float64 bins.  A cell whose float64 angle lies within heading_ref.EDGE_DEG of a bin edge is an edge cell:
the device's float32 acos may put it on the other side, so either neighbouring bin's table value is allowed there.

heading_predict in float64 (the fraction rounded once to float32, as the definition says):

    u = b - turn / (360 / nb), i0 = floor(u), f = (float)(u - i0)
    s(b) = (1 - f) hist[i0 mod nb] + f hist[(i0 + 1) mod nb]
    c = s circularly convolved with t[|j|], j = -r .. r
    v[b] = c(b) + floor (b < nb),  v[nb] = sum(c) / nb + floor,  out = log v"""
import numpy as np

from tests import heading_ref as hr

N = hr.N


def cell_bins(field, nb):
    """(k [N] in 0..nb: the table entry of every cell, other [N]: the entry an edge cell may take instead, edge [N] bool)"""
    k, edge = field.bins(nb)
    on = field.valid & (edge >= 0)
    other = np.where(edge == k, (k - 1) % nb, edge)          # the cell sits just above edge k, or just below edge (k + 1) % nb
    k = np.where(field.valid, k, nb)
    return k, np.where(on, other, k), on


def combined_map(field, table, nb, prior=None):
    """(comb float32 [N], alt float32 [N], edge bool [N]): the map, the value an edge cell may carry instead, and which cells are edge cells"""
    t = np.ascontiguousarray(table, dtype=np.float32)
    assert t.shape == (nb + 1,), t.shape
    k, other, edge = cell_bins(field, nb)
    comb, alt = t[k], t[other]
    if prior is not None:
        p = np.ascontiguousarray(prior, dtype=np.float32).reshape(N)
        with np.errstate(invalid="ignore"):                  # (-inf + inf)
            comb, alt = p + comb, p + alt                    # one float32 add
    return comb, alt, edge


def edge_share(field, nb):
    """share of the cells that are edge cells at nb bins"""
    return float(cell_bins(field, nb)[2].mean())


def same_bits(a, b):
    """elementwise: the same float32 bits, or both NaN"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return (a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))


def assert_map(got, field, table, nb, prior=None, what=""):
    """a device map [N] against the restatement: the same bits on every non-edge cell, one of the two allowed values on edge cells"""
    comb, alt, edge = combined_map(field, table, nb, prior)
    g = np.asarray(got, dtype=np.float32).reshape(N)
    first = same_bits(g, comb)
    bad = ~first & ~edge
    assert not bad.any(), f"{what}: {int(bad.sum())} non-edge cells differ, first at {int(np.argmax(bad))}: {g[bad][:4]} against {comb[bad][:4]}"
    bad = edge & ~first & ~same_bits(g, alt)
    assert not bad.any(), f"{what}: {int(bad.sum())} edge cells carry neither neighbour's value"
    assert edge.mean() <= hr.EDGE_CAP, f"{what}: {edge.mean():.3g} of the cells are edge cells"
    return int((edge & ~first).sum())


def predict(hist, turn_deg, taps, floor):
    """v float64 [B, nb + 1] of hist [B, nb], turn_deg [B] (float32 values), taps [r + 1] or [B, r + 1], floor [B]: out = log v"""
    h = np.asarray(hist, dtype=np.float64)
    B, nb = h.shape
    turn = np.broadcast_to(np.asarray(turn_deg, dtype=np.float32), (B,)).astype(np.float64)
    fl = np.broadcast_to(np.asarray(floor, dtype=np.float32), (B,)).astype(np.float64)
    t = np.asarray(taps, dtype=np.float32).astype(np.float64)
    t = np.broadcast_to(t, (B, t.shape[-1]))
    r = t.shape[1] - 1
    assert 2 * r + 1 <= nb
    v = np.empty((B, nb + 1))
    for q in range(B):
        with np.errstate(invalid="ignore"):
            u = np.arange(nb, dtype=np.float64) - turn[q] / (360.0 / nb)
            i0 = np.floor(u)
            f = (u - i0).astype(np.float32).astype(np.float64)
            if not np.isfinite(u).all():
                v[q] = np.nan
                continue
            i = np.mod(i0, nb).astype(np.int64)
            s = (1.0 - f) * h[q, i] + f * h[q, (i + 1) % nb]
        c = np.zeros(nb)
        for j in range(-r, r + 1):
            c += t[q, abs(j)] * np.roll(s, -j)               # c(b) += t[|j|] s[(b + j) mod nb]
        v[q, :nb] = c + fl[q]
        v[q, nb] = c.sum() / nb + fl[q]
    return v


def assert_predict(got, v, radius, what=""):
    """a device table [B, nb + 1] against predict()'s v: log(v - d) <= out <= log(v + d), d = (4 r + 12) 2^-24 v, each side widened by
    4 * 2^-24 * |log v| for logf; v == 0 (a zero hist without a floor) gives -inf exactly; a NaN row of v gives NaN"""
    g = np.asarray(got, dtype=np.float64)
    assert g.shape == v.shape, (g.shape, v.shape)
    nan = np.isnan(v)
    assert np.isnan(g[nan]).all(), f"{what}: NaN expected"
    zero = ~nan & (v == 0)
    assert (g[zero] == -np.inf).all(), f"{what}: -inf expected where the value is 0"
    m = ~nan & ~zero
    d = (4 * radius + 12) * 2.0 ** -24 * v[m]
    with np.errstate(divide="ignore"):
        lo, hi = np.log(v[m] - d), np.log(v[m] + d)
    slack = 4 * 2.0 ** -24 * np.abs(np.log(v[m]))
    ok = (g[m] >= lo - slack) & (g[m] <= hi + slack)
    worst = float(np.max(np.abs(g[m] - np.log(v[m])) / (hi - np.log(v[m]) + slack))) if m.any() else 0.0
    print(f"{what}: worst error / bound {worst:.3g}")
    assert ok.all(), f"{what}: {int((~ok).sum())} entries outside the bound, worst error / bound {worst:.3g}"
