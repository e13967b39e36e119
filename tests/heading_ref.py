"""float64 numpy restatement of the heading posterior (include/ccvpe.h), from a given float32 map h of 512 x 512 cells
and a float32 orientation field (c, s), and the tolerances a device result is held to.

A cell is valid when c and s are finite and not both zero.  Its angle is acos(clip(c, -1, 1)) in degrees, 360 minus that for s < 0
(the rule of rows[b][4]); bin b of nbins covers [b w, (b + 1) w), w = 360 / nbins, a result >= nbins wraps to b - nbins.

    hist[b]  sum of h over the valid cells of bin b
    0        M = sum of h over valid cells
    1, 2     C = sum h c / M, S = sum h s / M
    3        atan2(S, C) in degrees [0, 360); NaN when R == 0
    4        R = sqrt(C^2 + S^2)
    5        mode bin: first index of the maximal hist value; -1 for a query without a finite posterior
    6        hist[mode] / M
    7        M_w: M over the window |x - x*| <= radius, |y - y*| <= radius around the argmax of h, clipped to the grid
    8, 9     C_w, S_w over that window
    10, 11   mean heading and R of the window

A query without a finite posterior: heading NaN except column 5 = -1, hist zero.  Every sum is numpy's pairwise float64 sum.

Tolerances (from the formats, not from the device: assert_close):
    hist[b]        E_b + 2^-23 ref + 2^-33, E_b the mass of the cells whose float64 angle lies within EDGE_DEG of an edge of bin b (a
                   float32 acos may put those on the other side); 2^-23 ref covers the float32 result, 2^-33 the truncations of the
                   2^-52 fixed point (at most 262144 * 2^-52 = 2^-34 per bin)
    sum of hist    against column 0 within 2^-22
    0-2, 4, 6-9, 11   1e-6 absolute; the ratios only where their denominator (M, M_w) is >= 1e-6, NaN where it is 0
    3, 10          circular difference <= 1e-4 degree + degrees(1e-6 / R) where R >= 1e-3; NaN where R == 0 exactly
    5              exact, unless the two largest bins of the restatement differ by less than their tolerances"""
import numpy as np

HW = 512
N = HW * HW
COLS = 12
EDGE_DEG = 1e-3
EDGE_CAP = 0.01          # share of M the edge cells may hold in a test input (asserted from the restatement alone)
ABS = (0, 1, 2, 4, 6, 7, 8, 9, 11)
OVER_M, OVER_MW = (1, 2, 4, 6), (8, 9, 11)


class Field:
    """an orientation field [2, 512, 512] (float32) with what does not depend on the map: validity, angles, bins per bin count"""

    def __init__(self, ori):
        f = np.ascontiguousarray(ori, dtype=np.float32).reshape(2, N)
        self.c32, self.s32 = f[0], f[1]
        with np.errstate(invalid="ignore"):
            self.valid = np.isfinite(f[0]) & np.isfinite(f[1]) & ~((f[0] == 0) & (f[1] == 0))
            c = np.where(self.valid, f[0], 1.0).astype(np.float64)
            s = np.where(self.valid, f[1], 0.0).astype(np.float64)
            a = np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))
        self.c, self.s = c, s
        self.angle = np.where(s < 0, 360.0 - a, a)
        self._bins = {}

    def bins(self, nbins):
        """(bin of every cell, index of the edge every cell is within EDGE_DEG of or -1); edge e separates bins e - 1 and e"""
        if nbins not in self._bins:
            w = 360.0 / nbins
            k = np.floor(self.angle / w).astype(np.int64)
            d = self.angle - k * w
            k = np.where(k >= nbins, k - nbins, k)
            edge = np.where(d < EDGE_DEG, k, np.where(w - d < EDGE_DEG, (k + 1) % nbins, -1))
            self._bins[nbins] = (k, edge)
        return self._bins[nbins]


def _moments(h, c, s):
    with np.errstate(invalid="ignore", divide="ignore"):
        M = h.sum()
        C, S = (h * c).sum() / M, (h * s).sum() / M
        R = np.sqrt(C * C + S * S)
        mean = np.nan if not R > 0 else np.degrees(np.arctan2(S, C)) % 360.0
    return M, C, S, mean, R


def heading(h, field, nbins, radius, ok=True):
    """(row float64 [12], hist float64 [nbins], E float64 [nbins]) of one map h (float32, 512 * 512 values in any shape) over a Field;
    ok=False: the query has no finite posterior"""
    row = np.full(COLS, np.nan)
    if not ok:
        row[5] = -1
        return row, np.zeros(nbins), np.zeros(nbins)
    flat = np.ascontiguousarray(h, dtype=np.float32).reshape(-1)
    notnan = ~np.isnan(flat)
    idx = int(np.argmax(np.where(notnan, flat, -np.inf))) if notnan.any() else 0
    hv = np.where(field.valid, flat.astype(np.float64), 0.0)
    k, edge = field.bins(nbins)
    hist = np.bincount(k[field.valid], weights=hv[field.valid], minlength=nbins)
    on = field.valid & (edge >= 0)
    em = np.bincount(edge[on], weights=hv[on], minlength=nbins)
    E = em + np.roll(em, -1)                       # bin b lies between edges b and b + 1
    row[0:5] = _moments(hv, field.c, field.s)
    mode = int(np.argmax(hist))
    row[5] = mode
    with np.errstate(invalid="ignore", divide="ignore"):
        row[6] = hist[mode] / row[0]
    ys, xs = divmod(idx, HW)
    r = int(radius)
    y0, y1, x0, x1 = max(ys - r, 0), min(ys + r, HW - 1), max(xs - r, 0), min(xs + r, HW - 1)
    win = (slice(y0, y1 + 1), slice(x0, x1 + 1))
    row[7:12] = _moments(hv.reshape(HW, HW)[win], field.c.reshape(HW, HW)[win], field.s.reshape(HW, HW)[win])
    return row, hist, E


def circ_diff(a, b):
    d = np.abs(a - b) % 360.0
    return np.minimum(d, 360.0 - d)


def assert_edge_cap(row, E, what=""):
    """before any comparison: the cells a float32 angle may bin differently hold at most EDGE_CAP of the mass (every edge cell counts
    for the two bins it lies between)"""
    if row[0] > 0:
        assert E.sum() / 2.0 <= EDGE_CAP * row[0], f"{what}: edge cells hold {E.sum() / 2.0 / row[0]:.3g} of the mass"


def assert_close(got_row, got_hist, ref, what=""):
    """a device result (float32 [12], float32 [nbins]) against heading()'s (row, hist, E)"""
    row, hist, E = ref
    g, gh = np.asarray(got_row, dtype=np.float64), np.asarray(got_hist, dtype=np.float64)
    assert g.shape == (COLS,) and gh.shape == hist.shape, (g.shape, gh.shape, hist.shape)
    assert_edge_cap(row, E, what)
    assert np.isfinite(gh).all(), f"{what}: hist {gh}"
    if row[5] < 0:                                  # no posterior
        assert g[5] == -1 and np.isnan(np.delete(g, 5)).all() and (gh == 0).all(), f"{what}: empty row expected, got {g}, hist max {gh.max()}"
        return
    tol = E + 2.0 ** -23 * hist + 2.0 ** -33
    err = np.abs(gh - hist)
    assert (err <= tol).all(), f"{what}: hist bins {np.nonzero(err > tol)[0][:8]} off by {err[err > tol][:8]} (allowed {tol[err > tol][:8]})"
    assert abs(gh.sum() - g[0]) <= 2.0 ** -22, f"{what}: sum of hist {gh.sum()!r} against column 0 {g[0]!r}"
    checked = {0, 7}
    checked |= set(OVER_M) if row[0] >= 1e-6 else set()
    checked |= set(OVER_MW) if row[7] >= 1e-6 else set()
    worst = {}
    for col in sorted(checked):
        assert abs(g[col] - row[col]) <= 1e-6, f"{what}: column {col}: {g[col]!r} against {row[col]!r}"
        worst[col] = abs(g[col] - row[col]) / 1e-6
    for den, cols, mean in ((row[0], OVER_M, 3), (row[7], OVER_MW, 10)):
        if den == 0:
            assert np.isnan(g[list(cols) + [mean]]).all(), f"{what}: NaN ratios expected over a zero mass, got {g}"
    for mean, rr, den in ((3, 4, row[0]), (10, 11, row[7])):
        if den >= 1e-6 and row[rr] == 0:
            assert np.isnan(g[mean]), f"{what}: column {mean} must be NaN where R == 0, got {g[mean]!r}"
        elif den >= 1e-6 and row[rr] >= 1e-3:
            bound = 1e-4 + np.degrees(1e-6 / row[rr])
            d = circ_diff(g[mean], row[mean])
            assert d <= bound, f"{what}: column {mean}: {g[mean]!r} against {row[mean]!r} (allowed {bound:.3g})"
            assert 0.0 <= g[mean] < 360.0, f"{what}: column {mean} = {g[mean]!r} outside [0, 360)"
            worst[mean] = d / bound
    order = np.argsort(-hist, kind="stable")
    if hist[order[0]] - hist[order[1]] >= tol[order[0]] + tol[order[1]]:
        assert g[5] == row[5], f"{what}: mode {g[5]} against {row[5]}"
    else:
        assert 0 <= g[5] < len(hist) and g[5] == int(g[5]), f"{what}: mode {g[5]}"
    print(f"{what}: hist worst error / bound {float((err / tol).max()):.3g}; columns " + ", ".join(f"{c}: {v:.3g}" for c, v in worst.items()))


# ---- crafted fields ----------------------------------------------------------------------------------------------------------------

def unit_field(angle_deg):
    """float32 [2, 512, 512] (cos, sin) of angles in degrees (any shape that broadcasts to the grid), evaluated in float64"""
    a = np.radians(np.broadcast_to(np.asarray(angle_deg, dtype=np.float64), (HW, HW)))
    return np.stack([np.cos(a), np.sin(a)]).astype(np.float32)


def crafted_fields():
    """name -> float32 [2, 512, 512].  Crafted angles sit at the centres of the 360-bin grid (k + 0.5 degrees), which are interior
    points of every bin count the tests use (4, 20, 72, 360 bins: no edge is a multiple of 0.5 that is not a multiple of 1)."""
    rng = np.random.default_rng(77)
    yy, xx = np.mgrid[0:HW, 0:HW]
    special = unit_field(rng.uniform(0.0, 360.0, size=(HW, HW)))
    special[:, 5, 0:40] = np.nan                   # both components, one component, infinities, the zero vector
    special[0, 17, 100:130] = np.nan
    special[1, 60, 7:90] = np.inf
    special[0, 61, 7:90] = -np.inf
    special[:, 200:260, 300:380] = 0.0
    special[1, 300, 10:50] = -0.0                  # (c, -0): valid wherever c != 0
    special[0, 301, 10:50] = 0.0                   # (0, s): valid
    return {
        "constant": unit_field(123.5),
        "constant_wrap": unit_field(359.5),
        "random": unit_field(rng.uniform(0.0, 360.0, size=(HW, HW))),
        "random2": unit_field(rng.uniform(0.0, 360.0, size=(HW, HW))),
        "special": special,
        "two_mode": unit_field(np.where((xx + yy) % 3 == 0, 40.5, 220.5)),   # a street in both directions, one twice as likely
        "smooth": unit_field(0.5 + np.floor((xx * 0.6 + yy * 0.3) % 360.0)),    # slowly turning: long runs of one bin
    }
