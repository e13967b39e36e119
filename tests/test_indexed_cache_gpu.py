"""Indexed cached forms (ccvpe_*_cached_indexed, the tile_index keyword): a batch of queries against a cache of a few encoded
tiles must compute exactly what the unindexed cached calls compute on the explicitly gathered one-tile-per-query cache."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models, weights
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

EINVAL = -1
K, RADIUS = 8, 16
# the five encoder taps of the cache after the descriptor map: (pixels, channels) per sample (include/ccvpe.h, cache layout)
TAPS = [(256, 320), (1024, 112), (4096, 40), (16384, 24), (65536, 16)]


def make(variant, **kw):
    if variant == "vigor_ori_prior":
        m = models.CVM_VIGOR_ori_prior("cuda", 180.0, True, **kw)
    else:
        m = models.CVM_OxfordRobotCar("cuda", **kw)
    m.load_state_dict(weights.generate_state_dict(variant, 0))
    return m.to("cuda").eval()


def inputs(variant, batch, seed):
    g, s = weights.generate_inputs(variant, batch, seed, 360.0)
    return torch.from_numpy(g).cuda(), torch.from_numpy(s).cuda()


def gather_cache(m, cache, n_tiles, index):
    """The one-tile-per-query cache of `index` built in torch: every section of the documented layout
    [descriptor map T x 64 x D | tap sections T x HW x C], indexed along its sample axis.  D follows from the cache size."""
    per = _lib.load().ccvpe_aerial_cache_bytes(m._handle, 1) // 4
    rest = per - sum(hw * c for hw, c in TAPS)
    assert rest > 0 and rest % 64 == 0
    sizes = [rest] + [hw * c for hw, c in TAPS]
    assert cache.numel() == n_tiles * per
    idx = torch.as_tensor(np.asarray(index), dtype=torch.int64, device=cache.device)
    parts, o = [], 0
    for s in sizes:
        parts.append(cache[o:o + n_tiles * s].view(n_tiles, s)[idx].reshape(-1))
        o += n_tiles * s
    return torch.cat(parts)


def all_forms(m, g, cache, tile_index=None):
    """(nine outputs, rows, top-K rows) of the three cached forms"""
    kw = {} if tile_index is None else {"tile_index": tile_index}
    return (m.forward_cached(g, cache, **kw), m.localize_cached(g, cache, **kw), m.localize_topk_cached(g, cache, K, RADIUS, **kw))


def assert_forms_equal(got, ref, what):
    for i, (a, b) in enumerate(zip(got[0], ref[0])):
        assert torch.equal(a, b), f"{what}: {gu.OUTPUT_NAMES[i]} differs by {(a - b).abs().max().item():.3g}"
    assert torch.equal(got[1], ref[1]), f"{what}: rows"
    assert torch.equal(got[2], ref[2]), f"{what}: top-K rows"


@pytest.mark.parametrize("variant,precision", [("vigor_ori_prior", "fp32"), ("oxford", "fp32"), ("oxford", "bf16x3")])
def test_indexed_forms_equal_the_explicitly_gathered_cache(variant, precision):
    m = make(variant, precision=precision)
    index = [2, 0, 2, 1, 0]
    g, _ = inputs(variant, 5, 3)
    _, sat = inputs(variant, 3, 4)
    cache = m.encode_aerial(sat)
    got = all_forms(m, g, cache, index)
    ref = all_forms(m, g, gather_cache(m, cache, 3, index))
    assert_forms_equal(got, ref, f"{variant}/{precision}")
    # numpy and CPU-tensor indices are the same call
    assert torch.equal(m.localize_cached(g, cache, tile_index=np.array(index, np.int64)), ref[1])
    assert torch.equal(m.localize_cached(g, cache, tile_index=torch.tensor(index, dtype=torch.int32)), ref[1])


def test_more_queries_than_one_gather_launch_carries():
    """20 queries in one micro-batch: the copies split into launches of at most 16 samples (GATHER_MAX_SAMPLES)"""
    m = make("oxford")
    rng = np.random.default_rng(2)
    index = rng.integers(0, 3, size=20)
    g, _ = inputs("oxford", 20, 5)
    _, sat = inputs("oxford", 3, 6)
    cache = m.encode_aerial(sat)
    ref_cache = gather_cache(m, cache, 3, index)
    assert torch.equal(m.localize_cached(g, cache, tile_index=index), m.localize_cached(g, ref_cache))
    assert torch.equal(m.localize_topk_cached(g, cache, K, RADIUS, tile_index=index), m.localize_topk_cached(g, ref_cache, K, RADIUS))


def test_identity_index_equals_the_unindexed_calls():
    m = make("oxford")
    g, sat = inputs("oxford", 5, 8)
    cache = m.encode_aerial(sat)
    assert_forms_equal(all_forms(m, g, cache, list(range(5))), all_forms(m, g, cache), "identity index")


def test_micro_batch_loop_reads_each_slice_of_the_index():
    m = make("oxford", micro_batch=2)
    index = np.array([1, 0, 0, 1, 1])
    g, _ = inputs("oxford", 5, 9)
    _, sat = inputs("oxford", 2, 10)
    cache = m.encode_aerial(sat)
    got = all_forms(m, g, cache, index)
    slices = [all_forms(m, g[a:b], gather_cache(m, cache, 2, index[a:b])) for a, b in ((0, 2), (2, 4), (4, 5))]
    ref = ([torch.cat([s[0][i] for s in slices]) for i in range(9)], torch.cat([s[1] for s in slices]),
           torch.cat([s[2] for s in slices]))
    assert_forms_equal(got, ref, "micro_batch=2")
    # the cache may hold at most micro_batch tiles (what ccvpe_encode_aerial writes)
    big = gather_cache(m, cache, 2, [0, 1, 0])
    rows = torch.zeros(1, 5, device="cuda")
    idx = (C.c_int32 * 1)(2)
    assert _lib.load().ccvpe_localize_cached_indexed(m._handle, C.c_void_p(g.data_ptr()), 154, 231, C.c_void_p(big.data_ptr()), 3, idx, 1,
                                                     C.c_void_p(rows.data_ptr()), None) == EINVAL
    assert b"micro_batch" in _lib.load().ccvpe_last_error()
    # the keyword needs the tile count encode_aerial records
    with pytest.raises(ValueError, match="encode_aerial"):
        m.localize_cached(g[:1], big, tile_index=[2])


@pytest.mark.parametrize("variant", ["vigor_ori_prior", "oxford"])
def test_indexed_forward_matches_the_plain_forward(variant):
    """Not bitwise: the encode plan at batch T may run other tiles than the full plan at batch B.  The unit orientation field is
    compared weighted by the magnitude of its un-normalised vector (a debug run), as tests/test_parity_gpu.py does: F.normalize is
    ill-conditioned where that vector is ~0."""
    m = make(variant)
    index = [2, 0, 2, 1, 0]
    g, _ = inputs(variant, 5, 11)
    _, sat = inputs(variant, 3, 12)
    got = m.forward_cached(g, m.encode_aerial(sat), tile_index=index)
    sat_b = sat[torch.tensor(index, device=sat.device)]
    ref = m(g, sat_b)
    for name, a, b in zip(gu.OUTPUT_NAMES, got, ref):
        if name == "ori":
            continue
        fx = gu.summarize(name, b.cpu().numpy())
        gu.compare(name, fx, a.cpu().numpy(), 1e-4)
    md = make(variant)
    md.set_debug(True)
    md(g, sat_b)
    mag = md.read_tap("ori_level1_nchw").pow(2).sum(dim=1, keepdim=True).sqrt()
    err = ((got[2].cpu() - ref[2].cpu()).abs() * mag).max().item() / mag.max().item()
    assert err <= 1e-4, f"ori: magnitude-weighted error {err:.3g}"


def test_oxford_loop_end_to_end():
    """Resident uint8 map -> oxford_tiles -> window resize of the distinct tiles -> encode_aerial -> indexed localize_cached"""
    m = make("oxford")
    rng = np.random.default_rng(13)
    mp = torch.from_numpy(rng.integers(0, 256, size=(2400, 2800, 3), dtype=np.uint8)).cuda()
    # a drive of 12 frames over 3 tiles (x0 = 400, 800, 1200 at y0 = 800), the first one revisited
    xs = np.concatenate([np.linspace(610, 780, 4), np.linspace(1030, 1150, 3), np.linspace(1450, 1550, 3), [760.0, 700.0]])
    coords = np.stack([xs, np.full(12, 1000.0)], axis=1)
    t = aerial.oxford_tiles(coords)
    np.testing.assert_array_equal(t["origin"], [[400, 800], [800, 800], [1200, 800]])
    np.testing.assert_array_equal(t["tile_index"], [0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 0, 0])
    sat_t = aerial.oxford_tile_aerial(mp, t["origin"])
    # the per-tile preparation is the per-query one, deduplicated
    assert torch.equal(sat_t[torch.from_numpy(t["tile_index"]).long().cuda()], aerial.oxford_aerial(mp, coords))
    g, _ = inputs("oxford", 12, 14)
    cache = m.encode_aerial(sat_t)
    rows = m.localize_cached(g, cache, tile_index=t["tile_index"])
    ref = m.localize_cached(g, gather_cache(m, cache, 3, t["tile_index"]))
    assert torch.equal(rows, ref)
    gt = aerial.oxford_ground_truth(coords, np.zeros(12))
    assert gt["gt_index"].shape == (12,)


def test_refused_call_leaves_the_rows_untouched():
    m = make("oxford")
    g, _ = inputs("oxford", 3, 15)
    _, sat = inputs("oxford", 2, 16)
    cache = m.encode_aerial(sat)
    torch.cuda.synchronize()
    lib = _lib.load()
    rows = torch.full((3, K, 5), -7.25, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for bad in ((0, 2, 1), (0, -1, 1)):
        idx = (C.c_int32 * 3)(*bad)
        for rc in (lib.ccvpe_localize_cached_indexed(m._handle, C.c_void_p(g.data_ptr()), 154, 231, C.c_void_p(cache.data_ptr()), 2,
                                                     idx, 3, C.c_void_p(rows.data_ptr()), C.c_void_p(stream)),
                   lib.ccvpe_localize_topk_cached_indexed(m._handle, C.c_void_p(g.data_ptr()), 154, 231, C.c_void_p(cache.data_ptr()),
                                                          2, idx, 3, K, RADIUS, C.c_void_p(rows.data_ptr()), C.c_void_p(stream))):
            assert rc == EINVAL
            assert f"tile_index[1] = {bad[1]}".encode() in lib.ccvpe_last_error()
    torch.cuda.synchronize()
    assert bool((rows == -7.25).all())
    with pytest.raises(_lib.CcvpeError, match="tile_index"):
        m.localize_cached(g, cache, tile_index=[0, 2, 1])
    with pytest.raises(ValueError, match="host data"):
        m.localize_cached(g, cache, tile_index=torch.zeros(3, dtype=torch.int32, device="cuda"))
