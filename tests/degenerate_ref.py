"""numpy / float64 restatement of the rule for a sample without a finite posterior, and the crafted maps the
degenerate tests feed.

The five columns of a pose row from a stored map h (float32 [n]) and its orientation field (float32 [2, n]):

    taken     the values v of h with v > -inf; NaN compares false with everything, so it is never taken
    index     the first position of the largest taken value; -1 when nothing is taken (all NaN, all -inf, a mix of the two)
    prob      h[index]; NaN when nothing is taken
    cos, sin  the field at `index`, at pixel 0 when nothing is taken
    angle     pose_angle_deg(cos, sin)

This differs from numpy.argmax, which returns the first NaN of a map that holds one.  A form that takes logits answers the same rule
on the map its softmax would store, and that map is all NaN as soon as one logit is NaN or +inf or every logit is -inf: `finite`
below is tests/prior_ref.posterior's, and such a sample's row is (-1, NaN, cos0, sin0, angle0) whatever the other logits are.
"""
import numpy as np

from tests import prior_ref, topk_ref

HW = 512
N = HW * HW
CHUNK = N // 64          # values per workgroup of the post-processing kernels


def argmax_ref(h):
    """(index, prob) of one map under the rule: float32 values in any shape"""
    flat = np.ascontiguousarray(h, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        taken = flat > -np.inf
    if not taken.any():
        return -1, np.float32(np.nan)
    i = int(np.argmax(np.where(taken, flat, -np.inf)))          # numpy.argmax of a NaN-free array: the first maximal position
    return i, flat[i]


def rows_ref(heat, ori, angle=topk_ref.angle_deg):
    """rows float32 [B, 5] of heat [B, ...] (512 * 512 values each) and ori [B, 2, ...] under the contract; `angle` maps (cos, sin)
    arrays to the angle column"""
    heat = np.asarray(heat, np.float32)
    B = heat.shape[0]
    o = np.asarray(ori, np.float32).reshape(B, 2, -1)
    rows = np.zeros((B, 5), np.float32)
    for b in range(B):
        i, p = argmax_ref(heat[b])
        at = max(i, 0)
        rows[b, :4] = (i, p, o[b, 0, at], o[b, 1, at])
    rows[:, 4] = np.asarray(angle(rows[:, 2], rows[:, 3]), np.float32)
    return rows


def logits_rows_ref(logits, ori, log_prior=None, angle=topk_ref.angle_deg):
    """(rows float32 [B, 5], finite bool [B], h float64 [B, n]) of the forms that take logits: the rule on the posterior of
    tests/prior_ref.py, (-1, NaN) and pixel 0 for a sample whose softmax statistics are not finite"""
    lg = np.asarray(logits, np.float32).reshape(len(logits), -1)
    post = prior_ref.posterior(lg, np.zeros(lg.shape[1], np.float32) if log_prior is None else log_prior)
    B = lg.shape[0]
    o = np.asarray(ori, np.float32).reshape(B, 2, -1)
    rows = np.zeros((B, 5), np.float32)
    for b in range(B):
        if post["finite"][b]:
            i = int(np.argmax(post["h"][b]))
            rows[b, :4] = (i, post["h"][b, i], o[b, 0, i], o[b, 1, i])
        else:
            rows[b, :4] = (-1, np.nan, o[b, 0, 0], o[b, 1, 0])
    rows[:, 4] = np.asarray(angle(rows[:, 2], rows[:, 3]), np.float32)
    return rows, post["finite"], post["h"]


def metrics_ref(rows, heat, gt_index, meter_per_pixel):
    """(pixel_distance, meter_distance, prob_at_gt) float64 [B] of ccvpe_eval_metrics from the pose rows: NaN distances for index -1,
    NaN probability for a ground truth outside the map"""
    heat = np.asarray(heat, np.float32).reshape(len(rows), -1)
    B = len(rows)
    out = np.full((3, B), np.nan)
    mpp = np.broadcast_to(np.asarray(meter_per_pixel, np.float64), (B,))
    for b in range(B):
        pi, gi = int(rows[b, 0]), int(gt_index[b])
        if pi >= 0:
            py, px = divmod(pi, HW)
            gy = int(np.trunc(gi / HW))                 # C division truncates towards zero
            gx = gi - gy * HW
            out[0, b] = np.sqrt(float((gy - py) ** 2 + (gx - px) ** 2))
            out[1, b] = out[0, b] * mpp[b]
        if 0 <= gi < heat.shape[1]:
            out[2, b] = heat[b, gi]
    return out


# ---- the crafted batch -------------------------------------------------------------------------------------------------------------

CLASSES = ("ordinary0", "all_nan", "ordinary1", "all_neg_inf", "nan_neg_inf_mix", "ordinary2", "nan_at_0", "nan_at_last", "nan_beside_max",
           "ordinary3", "constant", "max_in_two_chunks", "max_in_two_lanes", "max_at_last", "ordinary4", "pos_inf")
HEAT_CLASSES = CLASSES[:-1]                  # one +inf among finite values is a class of the logits forms
ORDINARY = tuple(i for i, n in enumerate(CLASSES) if n.startswith("ordinary"))
NO_VALUE = ("all_nan", "all_neg_inf", "nan_neg_inf_mix")                                   # stored maps without a taken value
NO_POSTERIOR = NO_VALUE + ("nan_at_0", "nan_at_last", "nan_beside_max", "pos_inf")         # logits without finite statistics
PEAK = np.float32(12.0)


def _noise(rng):
    """positive noise below 1 with one clear peak: usable as a stored map (non-negative) and as logits (a posterior with one argmax
    that no rounding of the exponentials can move)"""
    h = rng.uniform(0.01, 1.0, size=N).astype(np.float32)
    at = int(rng.integers(0, N))
    h[at] = PEAK
    return h, at


def crafted_batch(seed=5):
    """(maps float32 [16, 512 * 512] in the order of CLASSES, want: name -> the index the rule gives a stored map by hand, or None
    where the noise decides it)"""
    rng = np.random.default_rng(seed)
    maps, want = [], {}
    for name in CLASSES:
        h, at = _noise(rng)
        if name.startswith("ordinary"):
            want[name] = at
        elif name == "all_nan":
            h[:] = np.nan
            want[name] = -1
        elif name == "all_neg_inf":
            h[:] = -np.inf
            want[name] = -1
        elif name == "nan_neg_inf_mix":
            h[:] = -np.inf
            h[rng.integers(0, N, size=N // 3)] = np.nan
            h[0], h[N - 1] = np.nan, -np.inf
            want[name] = -1
        elif name == "nan_at_0":
            h[at] = 0.5                      # (the peak may not sit at 0)
            at = 7 * CHUNK + 1234
            h[at] = PEAK
            h[0] = np.nan
            want[name] = at
        elif name == "nan_at_last":
            h[at] = 0.5
            at = 3 * CHUNK + 77
            h[at] = PEAK
            h[N - 1] = np.nan
            want[name] = at
        elif name == "nan_beside_max":
            h[at] = 0.5
            at = 40 * CHUNK + 4 * 301 + 2    # lane 2 of its float4; lanes 0, 1 and 3 hold NaN
            h[at - 2], h[at - 1], h[at + 1] = np.nan, np.nan, np.nan
            h[at] = PEAK
            want[name] = at
        elif name == "constant":
            h[:] = np.float32(0.25)
            want[name] = 0
        elif name == "max_in_two_chunks":
            h[at] = 0.5
            a, b = 50 * CHUNK + 4000, 9 * CHUNK + 4095     # the later chunk holds it at a lower offset; the earlier position wins
            h[a] = h[b] = PEAK
            want[name] = b
        elif name == "max_in_two_lanes":
            h[at] = 0.5
            q = 21 * CHUNK + 4 * 900
            h[q + 1] = h[q + 3] = PEAK
            want[name] = q + 1
        elif name == "max_at_last":
            h[at] = 0.5
            h[N - 1] = PEAK
            want[name] = N - 1
        elif name == "pos_inf":
            h[at] = 0.5
            h[100 * HW + 200] = np.inf
            want[name] = 100 * HW + 200      # as a stored map +inf is a value like any other; as a logit it leaves no posterior
        maps.append(h)
    return np.stack(maps), want


def unit_field(B, seed=6):
    """float32 [B, 2, 512, 512]: unit (cos, sin) of uniform random angles"""
    a = np.random.default_rng(seed).uniform(0.0, 2.0 * np.pi, size=(B, HW, HW))
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)
