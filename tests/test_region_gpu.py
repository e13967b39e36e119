"""One ground encoding per query against several aerial tiles (encode_ground + localize_region, ccvpe_localize_region): the pair
plan computes the bits of the indexed cached pose plan on an explicitly gathered ground cache, the cross-tile reduction is the
numpy restatement of tests/region_ref.py, and both agree with the full forward's logits."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models, weights
from tests import region_ref

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -2
VARIANTS = [("vigor_ori_prior", "fp32"), ("oxford", "fp32"), ("oxford", "bf16x3")]
UNEVEN = [[1], [0, 2, 1, 2], [2, 0]]   # 1, 4 and 2 tiles; shared and repeated ids


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


def flat(tiles):
    off = np.concatenate([[0], np.cumsum([len(t) for t in tiles])]).astype(np.int32)
    return off, np.concatenate([np.asarray(t, np.int32) for t in tiles])


def gathered_ground_cache(gcache, qop):
    """the ground cache of one query per pair, built in torch from the documented [G][Ltot] layout"""
    G = gcache._ccvpe_batch
    out = gcache.view(G, -1)[torch.as_tensor(qop, dtype=torch.int64, device=gcache.device)].reshape(-1).contiguous()
    out._ccvpe_batch = len(qop)
    out._ccvpe_grd_hw = gcache._ccvpe_grd_hw
    return out


@pytest.mark.parametrize("variant,precision", VARIANTS)
def test_encode_ground_matches_the_debug_forward_taps(variant, precision):
    m = make(variant, precision=precision)
    g, s = inputs(variant, 3, 1)
    gc = m.encode_ground(g).view(3, -1).cpu()
    md = make(variant, precision=precision)
    md.set_debug(True)
    md(g, s)
    o = 0
    for k in range(1, 7):
        tap = md.read_tap(f"grd_desc{k}").reshape(3, -1)
        L = tap.shape[1]
        got = gc[:, o:o + L]
        err = (got - tap).abs().max().item() / tap.abs().max().item()
        assert err <= 1e-5, f"grd_desc{k}: {err:.3g}"
        o += (L + 3) // 4 * 4
    assert o == gc.shape[1], "Ltot is the sum of the levels rounded up to 4"


@pytest.mark.parametrize("variant,precision", VARIANTS)
def test_identity_pairs_equal_the_indexed_cached_localize(variant, precision):
    m = make(variant, precision=precision)
    g, s = inputs(variant, 4, 2)
    gc, sc = m.encode_ground(g), m.encode_aerial(s)
    tiles = [2, 0, 3, 1]
    r = m.localize_region(gc, sc, [[t] for t in tiles])
    ref = m.localize_cached(g, sc, tile_index=tiles)
    assert torch.equal(r["pair_rows"], ref) and torch.equal(r["rows"], ref)
    assert bool((r["tile_prob"] == 1.0).all())
    assert torch.equal(r["pair"].cpu(), torch.arange(4, dtype=torch.int32))
    np.testing.assert_array_equal(r["pair_tile"], tiles)


@pytest.mark.parametrize("variant,precision", VARIANTS)
def test_uneven_lists_equal_the_gathered_ground_cache_and_the_numpy_reduction(variant, precision):
    m = make(variant, precision=precision)
    g, s = inputs(variant, 3, 3)
    gc, sc = m.encode_ground(g), m.encode_aerial(s)
    off, ft = flat(UNEVEN)
    qop = region_ref.query_of_pair(off)
    r = m.localize_region(gc, sc, UNEVEN)
    ref = m.localize_region(gathered_ground_cache(gc, qop), sc, [[t] for t in ft])
    assert torch.equal(r["pair_rows"], ref["pair_rows"])
    assert torch.equal(r["pair_stats"], ref["pair_stats"])
    # the cross-tile step against its numpy restatement on the returned per-pair values
    want = region_ref.region_reduce(off, r["pair_stats"].cpu().numpy(), r["pair_rows"].cpu().numpy())
    assert (want["margin"] > 1e-6).all(), want["margin"]
    np.testing.assert_array_equal(r["pair"].cpu().numpy(), want["best_pair"])
    rows = r["rows"].cpu().numpy()
    np.testing.assert_allclose(rows[:, 1], want["rows"][:, 1], rtol=1e-6)
    np.testing.assert_array_equal(rows[:, [0, 2, 3, 4]], want["rows"][:, [0, 2, 3, 4]])
    np.testing.assert_allclose(r["tile_prob"].cpu().numpy(), want["tile_prob"], rtol=1e-6)
    # the repeated tile of query 1 (pairs 2 and 4 both read tile 2): the same statistics, the same share
    assert torch.equal(r["pair_stats"][2], r["pair_stats"][4]) and r["tile_prob"][2] == r["tile_prob"][4]


@pytest.mark.parametrize("variant", ["vigor_ori_prior", "oxford"])
def test_statistics_and_joint_probability_match_the_full_forward(variant):
    m = make(variant)
    g, s = inputs(variant, 3, 4)
    gc, sc = m.encode_ground(g), m.encode_aerial(s)
    off, ft = flat(UNEVEN)
    qop = region_ref.query_of_pair(off)
    r = m.localize_region(gc, sc, UNEVEN)
    logits = m.forward_cached(g[torch.as_tensor(qop).cuda()], sc, tile_index=ft)[0].double().cpu().numpy()
    mx = logits.max(axis=1)
    inv = 1.0 / np.exp(logits - mx[:, None]).sum(axis=1)
    st = r["pair_stats"].double().cpu().numpy()
    assert np.abs(st[:, 0] - mx).max() <= 1e-4 * np.abs(mx).max()
    assert np.abs(st[:, 1] - inv).max() <= 1e-4 * np.abs(inv).max()
    rows, pair = r["rows"].cpu().numpy(), r["pair"].cpu().numpy()
    for q in range(len(UNEVEN)):
        lo, hi = off[q], off[q + 1]
        allv = logits[lo:hi].reshape(-1)
        lse = allv.max() + np.log(np.exp(allv - allv.max()).sum())
        p = int(pair[q])
        assert lo <= p < hi
        idx = int(rows[q, 0])
        joint = np.exp(logits[p, idx] - lse)
        assert abs(rows[q, 1] - joint) <= 1e-4 * joint, (q, rows[q, 1], joint)
        top2 = np.sort(logits[p])[-2:]
        if top2[1] - top2[0] > 1e-5:
            assert idx == int(np.argmax(logits[p]))


def test_micro_batch_loop_and_its_limits():
    lists = [[0, 1, 1], [1, 0, 0, 1]]   # P = 7 pairs: slices of 2, 2, 2, 1
    g, s = inputs("oxford", 2, 5)
    m2 = make("oxford", micro_batch=2)
    got = m2.localize_region(m2.encode_ground(g), m2.encode_aerial(s), lists)
    m = make("oxford")
    ref = m.localize_region(m.encode_ground(g), m.encode_aerial(s), lists)
    for k in ("rows", "pair_rows", "pair_stats", "tile_prob"):
        a, b = got[k].double(), ref[k].double()
        assert (a - b).abs().max().item() <= 1e-4 * max(b.abs().max().item(), 1e-30), k
    # the same tile wins; which of a query's repeats of it does is a tie the slices may break apart (pairs 3 and 6 run in one
    # batch-7 plan on the default handle, in plans of batch 2 and 1 here)
    np.testing.assert_array_equal(got["pair_tile"][got["pair"].cpu().numpy()], ref["pair_tile"][ref["pair"].cpu().numpy()])
    # the caches may hold at most micro_batch queries / tiles (what the encoders write)
    g3, s3 = inputs("oxford", 3, 6)
    gc3, sc3 = m.encode_ground(g3), m.encode_aerial(s3)
    gc2, sc2 = m2.encode_ground(g3[:2]), m2.encode_aerial(s3[:2])
    lib = _lib.load()
    outs = [torch.zeros(n, device="cuda") for n in (15, 3, 15, 6, 3)]
    ptrs = [C.c_void_p(t.data_ptr()) for t in outs]
    for gcache, nq, scache, nt, word in ((gc3, 3, sc2, 2, b"n_queries 3"), (gc2, 2, sc3, 3, b"n_tiles 3")):
        off = (C.c_int32 * (nq + 1))(*range(nq + 1))
        tl = (C.c_int32 * nq)(*([0] * nq))
        rc = lib.ccvpe_localize_region(m2._handle, C.c_void_p(gcache.data_ptr()), nq, 154, 231, C.c_void_p(scache.data_ptr()), nt, off, tl,
                                       *ptrs, None)
        assert rc == EINVAL and word in lib.ccvpe_last_error() and b"micro_batch" in lib.ccvpe_last_error()


def test_refused_calls_leave_the_outputs_untouched():
    m = make("oxford")
    g, s = inputs("oxford", 3, 7)
    gc, sc = m.encode_ground(g), m.encode_aerial(s)
    torch.cuda.synchronize()
    lib = _lib.load()
    outs = [torch.full((n,), -7.25, device="cuda") for n in (15, 3, 35, 14, 7)]
    ptrs = [C.c_void_p(t.data_ptr()) for t in outs]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(offsets, tiles, nq=3, nt=2, h=None):
        off = (C.c_int32 * len(offsets))(*offsets)
        tl = (C.c_int32 * len(tiles))(*tiles)
        rc = lib.ccvpe_localize_region(h or m._handle, C.c_void_p(gc.data_ptr()), nq, 154, 231, C.c_void_p(sc.data_ptr()), nt, off, tl,
                                       *ptrs, stream)
        return rc, (lib.ccvpe_last_error() or b"").decode()

    good = [0, 1, 5, 7], [0, 1, 1, 0, 1, 1, 0]
    cases = [(([1, 1, 5, 7], good[1]), "offsets[0] = 1"), (([0, 1, 1, 7], good[1]), "offsets[2] = 1"),
             (([0, 4, 2, 7], good[1]), "offsets[2] = 2"), ((good[0], [0, 1, 1, 0, 2, 1, 0]), "tiles[4] = 2"),
             ((good[0], [0, 1, -3, 0, 1, 1, 0]), "tiles[2] = -3")]
    for (o, t), word in cases:
        rc, msg = call(o, t)
        assert rc == EINVAL and word in msg, (word, msg)
    for nq, nt in ((0, 2), (3, 0)):
        rc, msg = call(*good, nq=nq, nt=nt)
        assert rc == EINVAL
    rc, msg = lib.ccvpe_localize_region(m._handle, None, 3, 154, 231, C.c_void_p(sc.data_ptr()), 2, (C.c_int32 * 4)(*good[0]),
                                        (C.c_int32 * 7)(*good[1]), *ptrs, stream), None
    assert rc == EINVAL
    md = make("oxford")
    md.set_debug(True)
    md.encode_aerial(s)   # the handle exists and is finalised
    rc, msg = call(*good, h=md._handle)
    assert rc == ESTATE and "debug" in msg
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == -7.25).all())
    with pytest.raises(ValueError, match="host data"):
        m.localize_region(gc, sc, [[0], torch.zeros(2, dtype=torch.int32, device="cuda"), [1]])
    with pytest.raises(_lib.CcvpeError, match="tiles"):
        m.localize_region(gc, sc, [[0], [1, 5], [1]])
    with pytest.raises(ValueError, match="queries"):
        m.localize_region(gc, sc, [[0], [1]])


@pytest.mark.parametrize("variant,G,per,pool", [("vigor_ori_prior", 1, 2, 2), ("oxford", 1, 2, 2), ("vigor_ori_prior", 32, 4, 32)])
def test_fresh_handle_measures_nothing(variant, G, per, pool, monkeypatch):
    """the committed tuning table alone covers the new plans (batch 1, 2 and four slices of 32 for VIGOR-ori-prior)"""
    monkeypatch.setenv("CCVPE_TUNE_CACHE", "off")
    m = make(variant)
    g, _ = inputs(variant, G, 8)
    _, s = inputs(variant, pool, 9)
    rng = np.random.default_rng(G)
    lists = [list(rng.choice(pool, size=per, replace=False)) for _ in range(G)]
    r = m.localize_region(m.encode_ground(g), m.encode_aerial(s), lists)
    torch.cuda.synchronize()
    assert _lib.load().ccvpe_tuning_generation(m._handle) == 0, "a launch missed the tuning table and was measured"
    assert torch.isfinite(r["rows"]).all() and r["pair_rows"].shape == (G * per, 5)


def test_repeated_calls_are_bit_equal():
    m = make("vigor_ori_prior")
    g, s = inputs("vigor_ori_prior", 3, 10)
    gc, sc = m.encode_ground(g), m.encode_aerial(s)
    rs = [m.localize_region(gc, sc, UNEVEN) for _ in range(3)]
    for r in rs[1:]:
        for k in ("rows", "pair", "pair_rows", "pair_stats", "tile_prob"):
            assert torch.equal(r[k], rs[0][k]), k


def test_oxford_region_loop_end_to_end():
    """resident uint8 map -> priors -> oxford_region -> window resize of the distinct tiles -> encode_aerial; uint8 ground frames ->
    preprocess -> encode_ground -> localize_region -> oxford_region_to_map"""
    m = make("oxford")
    rng = np.random.default_rng(11)
    mp = torch.from_numpy(rng.integers(0, 256, size=(2400, 2800, 3), dtype=np.uint8)).cuda()
    priors = np.array([[1000.0, 1000.0], [1150.0, 1020.0], [1650.0, 1400.0]])
    reg = aerial.oxford_region(priors, 400)
    assert reg["origin"].shape[0] <= 32
    sat = aerial.oxford_tile_aerial(mp, reg["origin"])
    sc = m.encode_aerial(sat)
    grd_u8 = torch.from_numpy(rng.integers(0, 256, size=(3, 154, 231, 3), dtype=np.uint8)).cuda()
    gc = m.encode_ground(_lib.preprocess(grd_u8))
    r = m.localize_region(gc, sc, reg["tiles"])
    own = aerial.oxford_window(priors)["origin"]
    for q in range(3):
        assert tuple(own[q]) in {tuple(reg["origin"][t]) for t in reg["tiles"][q]}
    rows, pair = r["rows"].cpu().numpy(), r["pair"].cpu().numpy()
    assert np.isfinite(rows).all() and np.isfinite(r["tile_prob"].cpu().numpy()).all()
    chosen = reg["origin"][r["pair_tile"][pair]]
    pos = aerial.oxford_region_to_map(chosen, rows[:, 0].astype(np.int64))
    assert ((pos >= chosen) & (pos < chosen + 800)).all()
