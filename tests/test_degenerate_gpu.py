"""The output-side entry points on maps without a finite posterior: one batch of 512 x 512 maps that stacks every
degenerate class of tests/degenerate_ref.py between ordinary maps, through each entry point that takes stored maps or logits.

Every row follows the restatement - exact on the index, the NaN pattern and the orientation lookup, the per-feature references
(prior_ref, summary_ref, heading_ref, topk_ref) at their own tolerances on the finite columns; every ordinary map's results are, bit
for bit, those it gets alone and in a batch of ordinary maps; a second call gives the same bits; the clean batch gives the same bits
before and after (ticket counters and scratch are back at rest); and the stored-map forms do the same at an address that is 4-byte
but not 16-byte aligned (the value-by-value path)."""
import numpy as np
import pytest
import torch

from ccvpe_amd import _lib
from tests import degenerate_ref as dr
from tests import heading_ref as hr
from tests import summary_ref as sr
from tests import topk_ref
from tests.test_localize_gpu import make
from tests.test_topk_gpu import device_angle

pytestmark = pytest.mark.gpu

N, HW = dr.N, dr.HW
K, R = 5, 4                      # top-K: hypotheses and suppression radius
RADIUS, BINS = 8, 72             # summary / heading window and histogram
HEAT_FORMS = ("postprocess", "postprocess_rows", "evaluate", "postprocess_topk", "belief_summary")
LOGITS_FORMS = ("postprocess_prior", "postprocess_summary", "postprocess_heading", "track_update_logits", "op_pose_rows")
MPP = 0.25


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    c.m = make("oxford")
    c.maps, c.want = dr.crafted_batch()
    c.ori = dr.unit_field(16)
    yy, xx = np.mgrid[0:HW, 0:HW].astype(np.float32)
    c.lp = np.full((16, HW, HW), -1.5, np.float32)          # a constant keeps the crafted ties; one ordinary query gets a broad bump
    c.lp[5] = -((xx - 256.0) ** 2 + (yy - 256.0) ** 2) / np.float32(2 * 200.0 ** 2)
    c.gt = np.array([c.want[n] if c.want[n] >= 0 else 1000 for n in dr.CLASSES], np.int32)
    c.gt[0], c.gt[2], c.gt[5], c.gt[1] = -5, N, 3 * HW + 4, N + 7     # outside the map on two ordinary queries and a degenerate one
    c.maps_d, c.ori_d, c.lp_d = (torch.from_numpy(a).cuda() for a in (c.maps, c.ori, c.lp))
    # references, computed once
    c.rows_heat = dr.rows_ref(c.maps, c.ori, angle=device_angle)
    c.metrics = dr.metrics_ref(c.rows_heat, c.maps, c.gt, MPP)
    c.topk = topk_ref.topk_rows(c.maps.reshape(16, HW, HW), c.ori, K, R, angle=device_angle)
    c.rows_lg, c.fin_lg, c.h_lg = dr.logits_rows_ref(c.maps, c.ori, None, angle=device_angle)
    c.rows_lp, c.fin_lp, c.h_lp = dr.logits_rows_ref(c.maps, c.ori, c.lp.reshape(16, N), angle=device_angle)
    c.fields = {}
    return c


def run(c, form, sel, misaligned=False):
    """the entry point `form` on the samples `sel` of the crafted batch -> a tuple of tensors with the batch as their first axis"""
    B, m = len(sel), c.m
    ix = torch.as_tensor(sel, device="cuda")
    x, ori, lp = c.maps_d[ix], c.ori_d[ix], c.lp_d[ix]
    if misaligned:
        flat = torch.empty(B * N + 1, dtype=torch.float32, device="cuda")
        off = flat[1:].view(B, N)
        off.copy_(x)
        x = off
        assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    else:
        assert x.data_ptr() % 16 == 0
    heat = x.view(B, 1, HW, HW)
    if form == "postprocess":
        d = m.postprocess(heat, ori)
        return tuple(d[k] for k in ("index", "prob", "cos", "sin", "angle_deg"))
    if form == "postprocess_rows":
        return (m.postprocess_rows(heat, ori),)
    if form == "evaluate":
        d = m.evaluate(heat, ori, c.gt[sel], MPP)
        return (d["index"],) + tuple(d[k] for k in m.METRIC_FIELDS)
    if form == "postprocess_topk":
        return (m.postprocess_topk(heat, ori, K, R),)
    if form == "belief_summary":
        return (m.belief_summary(x.view(B, HW, HW), RADIUS),)
    if form == "postprocess_prior":
        return (m.postprocess_prior(x, ori, lp),)
    if form == "postprocess_summary":
        return tuple(m.postprocess_summary(x, ori, None, radius=RADIUS, posterior=True))
    if form == "postprocess_heading":
        return tuple(m.postprocess_heading(x, ori, None, radius=RADIUS, bins=BINS, posterior=True))
    if form == "track_update_logits":
        return tuple(m.track_update_logits(x, ori, lp))
    if form == "op_pose_rows":          # the plain pose tail of ccvpe_localize (no prior, posterior or summary) on given logits
        m._ensure_handle(x.device)
        return (_lib.op_pose_rows(m._handle, x, ori),)
    raise AssertionError(form)


def bits(t):
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def same_bits(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and torch.equal(bits(x), bits(y)), f"{what}: output {k} differs"


def eq_nan(got, ref, what):
    """numpy arrays with the same values and NaN in the same places"""
    np.testing.assert_array_equal(np.asarray(got), np.asarray(ref), err_msg=what)


def check_logits_rows(rows, ref, finite, sel, what):
    """rows of a logits form against degenerate_ref.logits_rows_ref: index, orientation and NaN exact; the probability within
    1e-5 relative (a float32 __expf of an argument below 16 in magnitude and a float32 sum of 2^18 terms, against float64)"""
    for k, b in enumerate(sel):
        name = dr.CLASSES[b]
        assert finite[b] == (name not in dr.NO_POSTERIOR), name
        eq_nan(rows[k, [0, 2, 3, 4]], ref[b, [0, 2, 3, 4]], f"{what} {name}")
        if finite[b]:
            assert abs(rows[k, 1] - ref[b, 1]) <= 1e-5 * ref[b, 1], (what, name, rows[k, 1], ref[b, 1])
        else:
            assert rows[k, 0] == -1 and np.isnan(rows[k, 1]), (what, name, rows[k])


def check_map(post, h, finite, sel, what):
    """the stored posterior: within 1e-5 relative of the float64 one (as the probability above), all zero without a posterior"""
    for k, b in enumerate(sel):
        if finite[b]:
            assert (np.abs(post[k].reshape(-1) - h[b]) <= 1e-5 * h[b]).all(), (what, dr.CLASSES[b])
        else:
            assert (post[k] == 0).all(), (what, dr.CLASSES[b])


def check(c, form, got, sel):
    got = [t.cpu().numpy() for t in got]
    names = [dr.CLASSES[b] for b in sel]
    if form in ("postprocess", "postprocess_rows"):
        rows = np.stack([g.astype(np.float32) for g in got], axis=1) if form == "postprocess" else got[0]
        eq_nan(rows, c.rows_heat[sel], form)
        for k, n in enumerate(names):
            assert (rows[k, 0] == -1 and np.isnan(rows[k, 1])) == (n in dr.NO_VALUE), (form, n)
            assert rows[k, 0] == c.want[n]
    elif form == "evaluate":
        eq_nan(got[0], c.rows_heat[sel, 0].astype(np.int64), "evaluate index")
        px, mt, pg = c.metrics[:, sel]
        eq_nan(np.isnan(got[1]), np.isnan(px), "pixel_distance NaN")
        eq_nan(np.isnan(got[2]), np.isnan(mt), "meter_distance NaN")
        np.testing.assert_allclose(got[1], px, rtol=1e-14, atol=0)          # (float64 sqrt of an integer: a rounding at most)
        np.testing.assert_allclose(got[2], mt, rtol=1e-14, atol=0)
        eq_nan(got[3], pg, "prob_at_gt")
        for k, b in enumerate(sel):
            assert np.isnan(got[1][k]) == (names[k] in dr.NO_VALUE)
            assert np.isnan(got[3][k]) == (not 0 <= c.gt[b] < N or bool(np.isnan(c.maps[b, min(max(c.gt[b], 0), N - 1)])))
        # the predicted angle is the row's: float32 on the device, float64 acos here
        assert (np.abs(got[4] - c.rows_heat[sel, 4]) <= 1e-3).all()
    elif form == "postprocess_topk":
        eq_nan(got[0], c.topk[sel], form)
        for k, n in enumerate(names):
            if n in dr.NO_VALUE:
                eq_nan(got[0][k], np.tile(np.array([-1, 0, 0, 0, 0], np.float32), (K, 1)), n)
            else:
                assert got[0][k, 0, 0] == c.want[n], n          # the strongest peak is the argmax
    elif form == "belief_summary":
        s = got[0]
        for k, b in enumerate(sel):
            n = names[k]
            if n in dr.NO_VALUE:          # nothing taken: an in-map index (0), the map's value there, no moments
                assert s[k, 0] == 0 and s[k, 15] == (RADIUS + 1) ** 2, (n, s[k])
                eq_nan(s[k, 1], c.maps[b, 0], n)
                assert np.isnan(s[k, 3:15]).all() and not np.isfinite(s[k, 2]), (n, s[k])
            else:
                assert s[k, 0] == c.want[n], n
                sr.assert_rows_close(s[k:k + 1], sr.summary(c.maps[b], RADIUS)[None], f"belief_summary {n}")
    elif form == "postprocess_prior":
        check_logits_rows(got[0], c.rows_lp, c.fin_lp, sel, form)
    elif form == "op_pose_rows":
        check_logits_rows(got[0], c.rows_lg, c.fin_lg, sel, form)
    elif form == "track_update_logits":
        check_logits_rows(got[0], c.rows_lp, c.fin_lp, sel, form)
        check_map(got[1], c.h_lp, c.fin_lp, sel, form)
    elif form == "postprocess_summary":
        rows, summ, post = got
        check_logits_rows(rows, c.rows_lg, c.fin_lg, sel, form)
        check_map(post, c.h_lg, c.fin_lg, sel, form)
        eq_nan(summ[:, 0:2], rows[:, 0:2], "summary columns 0, 1")
        for k, b in enumerate(sel):
            if c.fin_lg[b]:
                sr.assert_rows_close(summ[k:k + 1], sr.summary(post[k], RADIUS)[None], f"{form} {names[k]}")
            else:
                assert summ[k, 0] == -1 and np.isnan(summ[k, 1:]).all(), (names[k], summ[k])
    elif form == "postprocess_heading":
        rows, head, hist, post = got
        check_logits_rows(rows, c.rows_lg, c.fin_lg, sel, form)
        check_map(post, c.h_lg, c.fin_lg, sel, form)
        for k, b in enumerate(sel):
            if b not in c.fields:
                c.fields[b] = hr.Field(c.ori[b])
            ok = bool(c.fin_lg[b])
            hr.assert_close(head[k], hist[k], hr.heading(post[k] if ok else None, c.fields[b], BINS, RADIUS, ok=ok), f"{form} {names[k]}")
            assert (head[k, 5] == -1) == (not ok)
    else:
        raise AssertionError(form)


CASES = [(f, False) for f in HEAT_FORMS + LOGITS_FORMS] + [(f, True) for f in HEAT_FORMS]


@pytest.mark.parametrize("form,misaligned", CASES, ids=[f + ("-misaligned" if mis else "") for f, mis in CASES])
def test_every_class_through(ctx, form, misaligned):
    c = ctx
    every = list(range(len(dr.HEAT_CLASSES if form in HEAT_FORMS else dr.CLASSES)))
    assert [dr.CLASSES[b] for b in every] == list(dr.HEAT_CLASSES if form in HEAT_FORMS else dr.CLASSES)
    clean = list(dr.ORDINARY)
    before = run(c, form, clean, misaligned)
    got = run(c, form, every, misaligned)
    check(c, form, got, every)                                           # every sample of every class, none exempt
    same_bits(run(c, form, every, misaligned), got, f"{form}: second call")
    same_bits(run(c, form, clean, misaligned), before, f"{form}: the clean batch after the degenerate one")
    same_bits(tuple(t[clean] for t in got), before, f"{form}: ordinary maps among degenerate ones")
    for k, b in enumerate(clean):
        same_bits(run(c, form, [b], misaligned), tuple(t[k:k + 1] for t in before), f"{form}: {dr.CLASSES[b]} alone")
