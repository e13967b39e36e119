"""tests/degenerate_ref.py, the restatement of the rule for a sample without a finite posterior, held to numpy.argmax and
the oracle's postprocess on finite maps - ties included - and pinned, class by class, to rows computed by hand."""
import numpy as np
import pytest
import torch

from oracle import ccvpe_oracle as orc
from tests import degenerate_ref as dr
from tests import topk_ref

N, HW, CHUNK = dr.N, dr.HW, dr.CHUNK


@pytest.fixture(scope="module")
def batch():
    maps, want = dr.crafted_batch()
    return maps, want, dr.unit_field(len(maps))


def finite_classes(maps):
    return [b for b in range(len(maps)) if np.isfinite(maps[b]).all()]


def test_the_batch_holds_every_class_once(batch):
    maps, want, ori = batch
    assert maps.shape == (16, N) and maps.dtype == np.float32 and ori.shape == (16, 2, HW, HW)
    assert len(set(dr.CLASSES)) == 16 and set(want) == set(dr.CLASSES) and dr.ORDINARY == (0, 2, 5, 9, 14)
    c = {n: maps[i] for i, n in enumerate(dr.CLASSES)}
    assert np.isnan(c["all_nan"]).all() and (c["all_neg_inf"] == -np.inf).all()
    mix = c["nan_neg_inf_mix"]
    assert np.isnan(mix).any() and (mix == -np.inf).any() and (np.isnan(mix) | (mix == -np.inf)).all()
    for name, at in (("nan_at_0", 0), ("nan_at_last", N - 1)):
        assert np.isnan(c[name][at]) and np.isnan(c[name]).sum() == 1
    nb = c["nan_beside_max"]
    q = want["nan_beside_max"] // 4 * 4
    assert np.isnan(nb[q:q + 4]).sum() == 3 and nb[want["nan_beside_max"]] == dr.PEAK
    assert (c["constant"] == c["constant"][0]).all()
    two = np.nonzero(c["max_in_two_chunks"] == dr.PEAK)[0]
    assert len(two) == 2 and two[0] // CHUNK != two[1] // CHUNK and two[0] % CHUNK > two[1] % CHUNK
    lanes = np.nonzero(c["max_in_two_lanes"] == dr.PEAK)[0]
    assert len(lanes) == 2 and lanes[0] // 4 == lanes[1] // 4
    assert np.argmax(c["max_at_last"]) == N - 1 and np.isposinf(c["pos_inf"]).sum() == 1
    for i in dr.ORDINARY:
        assert np.isfinite(maps[i]).all() and (maps[i] > 0).all() and (maps[i] == dr.PEAK).sum() == 1


def test_finite_maps_follow_numpy_argmax_and_the_oracle(batch):
    maps, want, ori = batch
    fin = finite_classes(maps)
    assert len(fin) == 5 + 4          # the ordinary maps, the constant map, the three placed maxima
    rows = dr.rows_ref(maps, ori)
    idx, prob, cs, sn, deg = orc.postprocess(torch.from_numpy(maps[fin]).view(-1, 1, HW, HW), torch.from_numpy(ori[fin]))
    for k, b in enumerate(fin):
        assert rows[b, 0] == np.argmax(maps[b]) == int(idx[k]), dr.CLASSES[b]
        assert rows[b, 1] == maps[b].max() == float(prob[k])
        assert rows[b, 2] == float(cs[k]) and rows[b, 3] == float(sn[k])
        assert abs(rows[b, 4] - float(deg[k])) <= 1e-3, (rows[b, 4], float(deg[k]))
    # ties: the first of the equal maxima, as numpy.argmax
    assert rows[dr.CLASSES.index("constant"), 0] == 0
    assert rows[dr.CLASSES.index("max_in_two_chunks"), 0] == 9 * CHUNK + 4095
    assert rows[dr.CLASSES.index("max_in_two_lanes"), 0] == 21 * CHUNK + 3601


def test_every_class_gives_the_row_computed_by_hand(batch):
    maps, want, ori = batch
    rows = dr.rows_ref(maps, ori)
    o = ori.reshape(16, 2, N)
    for b, name in enumerate(dr.CLASSES):
        i = want[name]
        assert rows[b, 0] == i, name
        if name in dr.NO_VALUE:
            assert i == -1 and np.isnan(rows[b, 1])
            assert rows[b, 2] == o[b, 0, 0] and rows[b, 3] == o[b, 1, 0]          # the orientation of pixel 0
        else:
            assert rows[b, 1] == maps[b, i] and not np.isnan(rows[b, 1])
            assert rows[b, 2] == o[b, 0, i] and rows[b, 3] == o[b, 1, i]
        assert rows[b, 4] == topk_ref.angle_deg(rows[b, 2], rows[b, 3])
    # NaN among finite values never wins, where numpy.argmax returns the first NaN
    for name in ("nan_at_0", "nan_at_last", "nan_beside_max"):
        b = dr.CLASSES.index(name)
        assert np.isnan(maps[b, np.argmax(maps[b])]) and rows[b, 1] == dr.PEAK
    assert rows[dr.CLASSES.index("pos_inf"), 1] == np.inf


def test_small_maps_by_hand():
    nan, inf = np.nan, np.inf
    cases = [([1, 3, 2, 3], 1), ([nan, 1, 2, nan], 2), ([nan, nan, nan, nan], -1), ([-inf, -inf, -inf, -inf], -1), ([nan, -inf, nan, -inf], -1),
             ([-inf, -3e38, -inf, nan], 1), ([5, 5, 5, 5], 0), ([0, 0, 0, 7], 3), ([1, inf, inf, 2], 1), ([-0.0, 0.0, -1, nan], 0)]
    for v, i in cases:
        got, p = dr.argmax_ref(np.array(v, np.float32))
        assert got == i, (v, got)
        assert np.isnan(p) if i < 0 else p == np.float32(v[i])


def test_logits_forms_lose_the_posterior_to_one_bad_logit(batch):
    maps, want, ori = batch
    rows, finite, h = dr.logits_rows_ref(maps, ori)
    o = ori.reshape(16, 2, N)
    for b, name in enumerate(dr.CLASSES):
        assert finite[b] == (name not in dr.NO_POSTERIOR), name
        if finite[b]:
            assert rows[b, 0] == want[name] and abs(h[b].sum() - 1.0) < 1e-12
            assert rows[b, 1] == np.float32(h[b, want[name]])
        else:
            assert rows[b, 0] == -1 and np.isnan(rows[b, 1]) and rows[b, 2] == o[b, 0, 0] and rows[b, 3] == o[b, 1, 0]
    # a prior of -inf everywhere takes the posterior of an ordinary sample too; a finite one keeps the index of a clear peak
    lp = np.zeros((16, N), np.float32)
    lp[0] = -np.inf
    lp[2] = -1.5
    rows2, finite2, _ = dr.logits_rows_ref(maps, ori, lp)
    assert not finite2[0] and rows2[0, 0] == -1 and finite2[2] and rows2[2, 0] == want["ordinary1"]


def test_metrics_follow_the_rows(batch):
    maps, want, ori = batch
    rows = dr.rows_ref(maps[:15], ori[:15])
    gt = np.array([want[n] if want[n] >= 0 else 1000 for n in dr.HEAT_CLASSES], np.int64)
    gt[0], gt[2], gt[5] = -5, N, 3 * HW + 4
    px, mt, pg = dr.metrics_ref(rows, maps[:15], gt, 0.5)
    for b, name in enumerate(dr.HEAT_CLASSES):
        assert np.isnan(px[b]) == np.isnan(mt[b]) == (name in dr.NO_VALUE), name
    assert np.isnan(pg[0]) and np.isnan(pg[2]) and pg[5] == maps[5, 3 * HW + 4]
    y, x = divmod(want["ordinary2"], HW)
    assert px[5] == np.sqrt((y - 3) ** 2 + (x - 4) ** 2) and mt[5] == 0.5 * px[5]
    assert px[9] == 0 and pg[9] == dr.PEAK
