"""Top-K pose hypotheses on the GPU: ccvpe_postprocess_topk against the numpy restatement (tests/topk_ref.py) on crafted
heatmaps, and ccvpe_localize_topk / ccvpe_localize_topk_cached bit-identical to forward + postprocess_topk in every plan form."""
import numpy as np
import pytest
import torch

from ccvpe_amd import _lib
from tests import topk_ref
from tests.test_localize_gpu import SINGLE, inputs, make

pytestmark = pytest.mark.gpu

HW = 512


def device_angle(cs, sn):
    """The angle column from (cos, sin) with pose_angle_deg's float32 operations, on the device."""
    c = torch.from_numpy(np.ascontiguousarray(cs, np.float32)).cuda()
    s = torch.from_numpy(np.ascontiguousarray(sn, np.float32)).cuda()
    ang = torch.acos(torch.clamp(c, -1.0, 1.0)) * 57.29577951308232
    neg = torch.fmod(-ang, 360.0)
    neg = torch.where(neg < 0, neg + 360.0, neg)
    return torch.where(s < 0, neg, ang).cpu().numpy()


def crafted_heatmaps(B, real, seed):
    """B maps cycling through: Gaussian bumps (several of equal height), exact ties, a plateau with zero regions, a mostly
    zero map, the real forward heatmap, and - once - a map with a NaN pixel."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:HW, 0:HW].astype(np.float32)
    maps = []
    for i in range(B):
        kind = i % 5
        if kind == 0:
            h = np.full((HW, HW), 1e-7, np.float32)
            for j in range(12):
                cy, cx = rng.integers(0, HW, 2)
                s = rng.uniform(3, 40)
                amp = np.float32(0.01) if j < 4 else np.float32(rng.uniform(0.001, 0.02))
                h = np.maximum(h, amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)).astype(np.float32))
        elif kind == 1:
            h = (rng.integers(0, 4, (HW, HW)) / np.float32(1000)).astype(np.float32)
            h[0, 0] = h[HW - 1, HW - 1] = h[0, HW - 1] = h[HW - 1, 0] = np.float32(0.004)   # corners at the top value
            h[100, 100:140:2] = np.float32(0.004)
        elif kind == 2:
            h = np.full((HW, HW), np.float32(2.0 ** -18), np.float32)
            h[50:120, 200:400] = 0.0
            h[300:310, 300:310] = np.float32(2.0 ** -17)
            h[450, 10] = np.float32(2.0 ** -16)
        elif kind == 3:
            h = np.zeros((HW, HW), np.float32)
            h[rng.integers(0, HW, 9), rng.integers(0, HW, 9)] = rng.uniform(0.1, 1, 9).astype(np.float32)
            h[5, 5] = -1.0
        else:
            h = real.copy()
        maps.append(h)
    if B > 2:
        maps[2][200, 201] = np.nan
        maps[2][64, 64] = np.nan
    return np.stack(maps)


def random_ori(B, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn((B, 2, HW, HW), generator=g)
    return (o / o.norm(dim=1, keepdim=True)).to(torch.float32)


@pytest.fixture(scope="module")
def vigor():
    return make("vigor_prior180_circ")


@pytest.fixture(scope="module")
def real_heatmap(vigor):
    g, s = inputs("vigor_prior180_circ", 1, seed=3)
    return vigor(g, s)[1][0, 0].cpu().numpy()


CASES = [(1, 0, 1), (5, 1, 3), (64, 4, 33), (64, 0, 3), (5, 32, 33), (1, 32, 3), (64, 32, 1), (5, 4, 1), (64, 1, 3), (1, 4, 33)]


@pytest.mark.parametrize("k,r,B", CASES)
def test_postprocess_topk_matches_restatement(vigor, real_heatmap, k, r, B):
    heat = crafted_heatmaps(B, real_heatmap, seed=k * 100 + r)
    ori = random_ori(B, seed=B + k)
    rows = vigor.postprocess_topk(torch.from_numpy(heat).cuda().view(B, 1, HW, HW), ori.cuda(), k, r)
    assert rows.shape == (B, k, 5) and rows.dtype == torch.float32
    ref = topk_ref.topk_rows(heat, ori.numpy(), k, r, angle=device_angle)
    ref = torch.from_numpy(ref).cuda()
    for b in range(B):
        assert torch.equal(rows[b], ref[b]), (b, (rows[b] != ref[b]).nonzero()[:5].tolist())


def test_postprocess_topk_k1_equals_postprocess_rows(vigor):
    g, s = inputs("vigor_prior180_circ", 3, seed=5)
    outs = vigor(g, s)
    ref = vigor.postprocess_rows(outs[1], outs[2])
    for r in (0, 1, 4, 32):
        assert torch.equal(vigor.postprocess_topk(outs[1], outs[2], 1, r), ref.view(3, 1, 5)), r


def topk_of_forward(m, g, s, k, r):
    outs = m(g, s)
    return m.postprocess_topk(outs[1], outs[2], k, r)


def assert_topk_equal(got, ref):
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert torch.equal(got, ref), (got != ref).nonzero()[:5].tolist()
    assert bool((got[:, 0, 0] >= 0).all())


def test_single_sample_configs_equal_forward_plus_postprocess_topk():
    assert len(SINGLE) == 5
    for name in SINGLE:
        m = make(name)
        g, s = inputs(name, 2)
        assert_topk_equal(m.localize_topk(g, s, 8, 16), topk_of_forward(m, g, s, 8, 16))


def test_headline_batch32_and_committed_table_covers_topk_plan():
    m = make("vigor_prior180_circ")
    g, s = inputs("vigor_prior180_circ", 32, seed=11)
    rows = m.localize_topk(g, s, 8, 16)   # first call on a fresh handle: builds the top-K plan from the committed tuning table
    assert _lib.load().ccvpe_tuning_generation(m._handle) == 0, "a top-K plan launch missed the tuning table and was measured"
    outs = m(g, s)
    assert_topk_equal(rows, m.postprocess_topk(outs[1], outs[2], 8, 16))
    for k, r in ((64, 0), (5, 32), (1, 1)):   # one plan serves every (k, r)
        assert_topk_equal(m.localize_topk(g, s, k, r), m.postprocess_topk(outs[1], outs[2], k, r))


def test_k1_equals_localize_and_row0_equals_localize():
    m = make("vigor_prior180_circ")
    g, s = inputs("vigor_prior180_circ", 4, seed=37)
    ref = m.localize(g, s)
    assert torch.equal(m.localize_topk(g, s, 1, 0), ref.view(4, 1, 5))
    assert torch.equal(m.localize_topk(g, s, 1, 32), ref.view(4, 1, 5))
    assert torch.equal(m.localize_topk(g, s, 8, 16)[:, 0], ref)


def test_cached_aerial_equals_full_and_uncached():
    m = make("oxford")
    g, s = inputs("oxford", 1, seed=17)
    cache = m.encode_aerial(s)
    rows = m.localize_topk_cached(g, cache, 8, 16)
    outs = m.forward_cached(g, cache)
    assert_topk_equal(rows, m.postprocess_topk(outs[1], outs[2], 8, 16))
    assert_topk_equal(rows, m.localize_topk(g, s, 8, 16))
    assert torch.equal(rows[:, 0], m.localize_cached(g, cache))
    g2 = torch.roll(g, 37, dims=3)
    rows2 = m.localize_topk_cached(g2, cache, 3, 4)
    outs2 = m.forward_cached(g2, cache)
    assert_topk_equal(rows2, m.postprocess_topk(outs2[1], outs2[2], 3, 4))


def test_single_stream_gives_the_same_rows():
    g, s = inputs("vigor_prior180_circ", 2, seed=19)
    m = make("vigor_prior180_circ")
    two = m.localize_topk(g, s, 8, 16)
    m.set_streams(1)
    assert_topk_equal(m.localize_topk(g, s, 8, 16), two)


def test_unfused_level1_fallback(monkeypatch):
    monkeypatch.setenv("CCVPE_FUSE_L1", "0")   # read at ccvpe_create
    m = make("vigor_prior180_circ")
    g, s = inputs("vigor_prior180_circ", 2, seed=23)
    assert_topk_equal(m.localize_topk(g, s, 8, 16), topk_of_forward(m, g, s, 8, 16))
    assert_topk_equal(m.localize_topk(g, s, 64, 1), topk_of_forward(m, g, s, 64, 1))


def test_micro_batch_loop():
    m = make("vigor_prior180_circ", micro_batch=8)
    g, s = inputs("vigor_prior180_circ", 11, seed=13)   # 8 + 3
    assert_topk_equal(m.localize_topk(g, s, 5, 8), topk_of_forward(m, g, s, 5, 8))


def test_debug_handle_refuses_localize_topk():
    m = make("oxford")
    g, s = inputs("oxford", 1)
    m.set_debug(True)
    with pytest.raises(_lib.CcvpeError, match=r"\(-2\)"):
        m.localize_topk(g, s, 8, 16)
