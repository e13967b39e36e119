"""Pose-only forward (ccvpe_localize / ccvpe_localize_cached): the [B, 5] result rows must be bit-identical to what
postprocess_rows reads from the full forward's heatmap and orientation field, in every plan form the handle can run."""
import pytest
import torch

from ccvpe_amd import _lib, models, weights
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

SINGLE = [n for n, c in gu.CONFIGS.items() if c["batch"] == 1]


def make(name, **kw):
    cfg = gu.CONFIGS[name]
    v = cfg["variant"]
    if v == "vigor_ori_prior":
        m = models.CVM_VIGOR_ori_prior("cuda", cfg["ori_noise"], cfg["circular"], **kw)
    elif v == "vigor":
        m = models.CVM_VIGOR("cuda", cfg["circular"], **kw)
    elif v == "kitti":
        m = models.CVM_KITTI("cuda", **kw)
    else:
        m = models.CVM_OxfordRobotCar("cuda", **kw)
    m.load_state_dict(weights.generate_state_dict(v, cfg["seed"]))
    return m.to("cuda").eval()


def inputs(name, batch, seed=7):
    cfg = gu.CONFIGS[name]
    g, s = weights.generate_inputs(cfg["variant"], batch, seed, cfg["fov"])
    return torch.from_numpy(g).cuda(), torch.from_numpy(s).cuda()


def rows_of_forward(m, g, s):
    outs = m(g, s)
    return m.postprocess_rows(outs[1], outs[2])


def assert_rows_equal(got, ref):
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert torch.equal(got, ref), (got - ref).abs().max().item()
    idx = got[:, 0]
    assert bool(((idx >= 0) & (idx < 512 * 512)).all())


def test_single_sample_configs_equal_forward_plus_postprocess():
    assert len(SINGLE) == 5
    for name in SINGLE:
        m = make(name)
        g, s = inputs(name, 2)
        assert_rows_equal(m.localize(g, s), rows_of_forward(m, g, s))


def test_headline_batch32_and_committed_table_covers_pose_plan():
    m = make("vigor_prior180_circ")
    g, s = inputs("vigor_prior180_circ", 32, seed=11)
    rows = m.localize(g, s)   # first call on a fresh handle: builds the pose plan from the committed tuning table
    lib = _lib.load()
    assert lib.ccvpe_tuning_generation(m._handle) == 0, "a pose-plan launch missed the tuning table and was measured"
    assert_rows_equal(rows, rows_of_forward(m, g, s))


def test_micro_batch_loop():
    m = make("vigor_prior180_circ", micro_batch=8)
    g, s = inputs("vigor_prior180_circ", 19, seed=13)   # 8 + 8 + 3
    assert_rows_equal(m.localize(g, s), rows_of_forward(m, g, s))


def test_cached_aerial_equals_full_and_uncached():
    m = make("oxford")
    g, s = inputs("oxford", 1, seed=17)
    cache = m.encode_aerial(s)
    rows = m.localize_cached(g, cache)
    outs = m.forward_cached(g, cache)
    assert_rows_equal(rows, m.postprocess_rows(outs[1], outs[2]))
    assert_rows_equal(rows, m.localize(g, s))
    g2 = torch.roll(g, 37, dims=3)   # a second ground frame against the same cached tile
    rows2 = m.localize_cached(g2, cache)
    outs2 = m.forward_cached(g2, cache)
    assert_rows_equal(rows2, m.postprocess_rows(outs2[1], outs2[2]))


def test_single_stream_and_plan_order_issue_give_the_same_rows(monkeypatch):
    g, s = inputs("vigor_prior180_circ", 2, seed=19)
    m = make("vigor_prior180_circ")
    two = m.localize(g, s)
    m.set_streams(1)
    assert_rows_equal(m.localize(g, s), two)
    monkeypatch.setenv("CCVPE_ISSUE_ORDER", "0")   # read at ccvpe_create
    m2 = make("vigor_prior180_circ")
    assert_rows_equal(m2.localize(g, s), two)


def test_unfused_level1_fallback(monkeypatch):
    monkeypatch.setenv("CCVPE_FUSE_L1", "0")   # read at ccvpe_create
    m = make("vigor_prior180_circ")
    g, s = inputs("vigor_prior180_circ", 2, seed=23)
    assert_rows_equal(m.localize(g, s), rows_of_forward(m, g, s))


def test_bf16x3_precision():
    m = make("vigor_prior180_circ", precision="bf16x3")
    g, s = inputs("vigor_prior180_circ", 2, seed=29)
    assert_rows_equal(m.localize(g, s), rows_of_forward(m, g, s))


def test_localize_between_forwards_leaves_forward_outputs_unchanged():
    m = make("vigor_prior180_circ")
    g, s = inputs("vigor_prior180_circ", 2, seed=31)
    first = [t.clone() for t in m(g, s)]
    rows = m.localize(g, s)
    second = m(g, s)
    for i, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(a, b), gu.OUTPUT_NAMES[i]
    assert_rows_equal(rows, m.postprocess_rows(second[1], second[2]))


def test_debug_handle_refuses_localize():
    m = make("oxford")
    g, s = inputs("oxford", 1)
    m.set_debug(True)
    with pytest.raises(_lib.CcvpeError, match=r"\(-2\)"):
        m.localize(g, s)
