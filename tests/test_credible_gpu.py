"""Credible regions on the device (ccvpe_*_credible): the stored-map form gives the bits of the sorting restatement
tests/credible_ref.py - every column, every byte of the level map - on the crafted maps, at a misaligned address and on the special
maps; the logits and network forms give the rows and the map of the track_update forms and the stored-map form's bits on that map,
with or without it; a query without a posterior gets the all-zero map's row; the forms add exactly the stored-map form's launches and
measure nothing; the trackers append the cred of the belief they store."""
import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial
from tests import credible_ref as cr
from tests import test_summary_gpu as tsg

pytestmark = pytest.mark.gpu

N = 512 * 512
LEVELS = cr.LEVELS
make, inputs, gaussians, logits_case = tsg.make, tsg.inputs, tsg.gaussians, tsg.logits_case
MAPS = tsg.MAPS
_REFS = {}


def eq(a, b):
    assert a.shape == b.shape and torch.equal(a, b)


def eq_bits(a, b):
    """the same bits, NaN included"""
    assert a.shape == b.shape and a.dtype == b.dtype
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), (a, b)


def against_ref(cred, lmap, maps, probes, what, levels=LEVELS):
    """device results against the restatement of `maps` (numpy [B, 512, 512]), bit for bit"""
    want, wmap = cr.credibles(maps, levels, probes, level_map=True)
    got = cred.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    bad = np.argwhere(cr.bits(got) != cr.bits(want))
    assert bad.size == 0, (what, bad[:8].tolist(), got[bad[0, 0]], want[bad[0, 0]])
    if lmap is not None:
        g = lmap.cpu().numpy().reshape(len(maps), N)
        assert g.dtype == np.uint8 and (g == wmap).all(), (what, int((g != wmap).sum()))


def probes_for(names):
    """a cell of the first map's peak, a zero cell of the second (its smallest value where it has no zero), and -1"""
    return [int(np.argmax(MAPS[names[0]])), int(np.argmin(MAPS[names[1]])), -1]


def crafted(names):
    if names not in _REFS:
        _REFS[names] = cr.credibles(np.stack([MAPS[n] for n in names]), LEVELS, probes_for(names), level_map=True)
    return _REFS[names]


# ---- 1. stored maps --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("names", tsg.BATCHES)
def test_stored_maps_give_the_restatements_bits(names):
    m = make("oxford")
    maps = np.stack([MAPS[n] for n in names])
    probes = probes_for(names)
    want, wmap = crafted(names)
    bel = torch.from_numpy(maps).cuda()
    cred, lmap = m.belief_credible(bel, LEVELS, probes, level_map=True)
    assert cred.shape == (3, 4 + 3 * len(LEVELS)) and cred.dtype == torch.float32 and lmap.shape == (3, 512, 512) and lmap.dtype == torch.uint8
    eq_bits(cred, torch.from_numpy(want).cuda())
    assert torch.equal(lmap.view(3, N), torch.from_numpy(wmap).cuda()), names
    eq_bits(m.belief_credible(bel.view(3, 1, 512, 512), LEVELS, torch.tensor(probes, device="cuda")), cred)     # no level map: the same row
    again, lmap2 = m.belief_credible(bel, LEVELS, probes, level_map=True)                                      # and again: nothing left behind
    eq_bits(again, cred)
    assert torch.equal(lmap2, lmap)
    # without a probe: NaN in its two columns, everything else as before
    plain = m.belief_credible(bel, LEVELS)
    assert bool(torch.isnan(plain[:, 2:4]).all())
    eq_bits(plain[:, [0, 1] + list(range(4, plain.shape[1]))], cred[:, [0, 1] + list(range(4, plain.shape[1]))])
    # a 4-byte but not 16-byte aligned address (maps and level map): the value-by-value path adds the same integers
    flat = torch.empty(3 * N + 1, dtype=torch.float32, device="cuda")
    off = flat[1:].view(3, 512, 512)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    off.copy_(bel)
    c2, l2 = m.belief_credible(off, LEVELS, probes, level_map=True)
    eq_bits(c2, cred)
    assert torch.equal(l2, lmap)
    c3, l3 = m.belief_credible(off, LEVELS, probes, level_map=True)
    eq_bits(c3, c2)
    assert torch.equal(l3, l2)
    # levels in another order, one repeated: every level's columns are its own, the map counts them all
    other = (1.0, 0.5, 0.5)
    c4, l4 = m.belief_credible(bel, other, probes, level_map=True)
    against_ref(c4, l4, maps, probes, f"{names} levels {other}", other)


# ---- 2. special maps -------------------------------------------------------------------------------------------------------------

def test_special_maps():
    m = make("oxford")
    zero = np.zeros((512, 512), np.float32)
    odd = MAPS["random"].copy()
    odd[10, 20] = np.nan
    odd[400, 17] = 2.0
    tiny = np.full((512, 512), np.float32(2.0 ** -50))
    tiny[3, 3] = np.float32(2.0 ** -45)
    inf = MAPS["gauss_centre"].copy()
    inf[100, 200] = np.inf
    maps = np.stack([zero, odd, tiny, inf])
    probes = [5, 400 * 512 + 17, N, 100 * 512 + 200]          # N: the first index outside the map
    cred, lmap = m.belief_credible(torch.from_numpy(maps).cuda(), LEVELS, probes, level_map=True)
    against_ref(cred, lmap, maps, probes, "special maps")
    got = cred.cpu().numpy()
    lv = got[:, 4:].reshape(4, len(LEVELS), 3)
    for q in (0, 2):                                            # no mass: the documented empty rows, an all-zero level map
        assert got[q, 0] == 0 and np.isnan(lv[q, :, 0]).all() and (lv[q, :, 1] == 0).all() and np.isnan(lv[q, :, 2]).all()
        assert not bool(lmap[q].any())
    assert got[0, 1] == 0 and np.isnan(got[0, 2]) and got[0, 3] == 0
    assert got[2, 1] == N and np.isnan(got[2, 2:4]).all()      # keys without mass; the probe outside the map reads nothing
    assert got[1, 1] == N - 1 and got[1, 3] == 0 and got[1, 2] == 0          # the NaN cell has no key; 2.0 is the largest value
    assert np.isinf(lv[3, -1, 0]) and lv[3, -1, 1] == 1 and got[3, 3] == 0   # +inf is a value: the 1e-6 region is that one cell


# ---- 3. the logits form ----------------------------------------------------------------------------------------------------------

def test_logits_form_is_track_update_logits_plus_the_credible_rows_of_its_map():
    m = make("oxford")
    lg, ori = logits_case()
    lp = gaussians(3, 5, sigma=80.0)
    for prior in (lp, None):
        want_rows, want_map = m.track_update_logits(lg, ori, prior)
        probes = [int(want_rows[0, 0].item()), 0, -1]
        rows, cred, lmap, post = m.postprocess_credible(lg, ori, LEVELS, prior, probes, level_map=True, posterior=True)
        assert rows.shape == (3, 5) and cred.shape == (3, 4 + 3 * len(LEVELS)) and lmap.shape == (3, 512, 512) and post.shape == (3, 512, 512)
        eq(rows, want_rows)
        eq(post, want_map)
        wc, wl = m.belief_credible(post, LEVELS, probes, level_map=True)
        eq_bits(cred, wc)
        assert torch.equal(lmap, wl)
        against_ref(cred, lmap, post.cpu().numpy(), probes, f"logits prior={prior is not None}")
        rows2, cred2 = m.postprocess_credible(lg, ori, LEVELS, prior, probes)              # without either map: the same bits
        eq(rows2, rows)
        eq_bits(cred2, cred)
        rows3, cred3, lmap3 = m.postprocess_credible(lg, ori, LEVELS, prior, probes, level_map=True)
        eq_bits(cred3, cred)
        assert torch.equal(lmap3, lmap)
        assert cred[0, 3].item() == 0 and cred[0, 2].item() == 0                           # nothing lies above the argmax


def test_query_without_a_posterior_gets_the_zero_maps_row():
    m = make("oxford")
    lg, ori = logits_case()
    lp = gaussians(3, 6)
    probes = [17, 18, 19]
    ok = m.postprocess_credible(lg, ori, LEVELS, lp, probes, level_map=True, posterior=True)
    lp[1] = float("-inf")
    rows, cred, lmap, post = m.postprocess_credible(lg, ori, LEVELS, lp, probes, level_map=True, posterior=True)
    assert rows[1, 0].item() == -1 and torch.isnan(rows[1, 1]) and bool((post[1] == 0).all())
    zc, zl = m.belief_credible(torch.zeros(1, 512, 512, device="cuda"), LEVELS, [18], level_map=True)
    eq_bits(cred[1:2], zc)
    assert not bool(lmap[1].any()) and not bool(zl.any())
    for q in (0, 2):
        eq(rows[q], ok[0][q])
        eq_bits(cred[q], ok[1][q])
        assert torch.equal(lmap[q], ok[2][q])
        eq(post[q], ok[3][q])
    eq_bits(m.postprocess_credible(lg, ori, LEVELS, lp, probes)[1], cred)


# ---- 4. the network forms --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["oxford", "vigor_circ"])
def test_network_forms_are_track_update_plus_the_credible_rows_of_its_map(name):
    m = make(name)
    g, s = inputs(name, 2)
    lp = gaussians(2, 1)
    probes = [100 * 512 + 100, -1]
    want_rows, want_map = m.track_update(g, s, lp)
    rows, cred, lmap, post = m.localize_credible(g, s, LEVELS, lp, probes, level_map=True, posterior=True)
    eq(rows, want_rows)
    eq(post, want_map)
    wc, wl = m.belief_credible(post, LEVELS, probes, level_map=True)
    eq_bits(cred, wc)
    assert torch.equal(lmap, wl)
    rows2, cred2 = m.localize_credible(g, s, LEVELS, lp, probes)                        # without the maps
    eq(rows2, rows)
    eq_bits(cred2, cred)
    r0, c0, p0 = m.localize_credible(g, s, LEVELS, posterior=True)                     # no prior, no probe
    n0, m0 = m.track_update(g, s)
    eq(r0, n0)
    eq(p0, m0)
    eq_bits(c0, m.belief_credible(p0, LEVELS))
    sc = m.encode_aerial(s)
    for tiles in (None, [1, 1]):
        r1, c1, l1, p1 = m.localize_credible_cached(g, sc, LEVELS, lp, probes, level_map=True, posterior=True, tile_index=tiles)
        nr, nm = m.track_update_cached(g, sc, lp, tile_index=tiles)
        eq(r1, nr)
        eq(p1, nm)
        bc, bl = m.belief_credible(p1, LEVELS, probes, level_map=True)
        eq_bits(c1, bc)
        assert torch.equal(l1, bl)
        eq_bits(m.localize_credible_cached(g, sc, LEVELS, lp, probes, tile_index=tiles)[1], c1)


def test_micro_batch_slices_write_their_own_rows():
    """a micro_batch=2 handle runs three queries as slices of 2 + 1: every slice reads its own prior and probe and writes its own
    rows, cred, level map and posterior - the bits of the same handle's calls on the two slices"""
    name = "vigor_prior180_circ"
    m2 = make(name, micro_batch=2)
    g, s = inputs(name, 3, seed=53)
    lp = gaussians(3, 4, sigma=3.0)
    probes = [11, 22 * 512, 33]
    rows, cred, lmap, post = m2.localize_credible(g, s, LEVELS, lp, probes, level_map=True, posterior=True)
    bc, bl = m2.belief_credible(post, LEVELS, probes, level_map=True)
    eq_bits(cred, bc)
    assert torch.equal(lmap, bl)
    for sl in (slice(0, 2), slice(2, 3)):
        ra, ca, la, pa = m2.localize_credible(g[sl], s[sl], LEVELS, lp[sl].contiguous(), probes[sl], level_map=True, posterior=True)
        eq(rows[sl], ra)
        eq_bits(cred[sl], ca)
        assert torch.equal(lmap[sl], la)
        eq(post[sl], pa)


# ---- 5. launches and tuning ------------------------------------------------------------------------------------------------------

def test_credible_forms_add_the_stored_map_forms_launches_and_measure_nothing():
    lib = _lib.load()
    m = make("oxford")
    g, s = inputs("oxford", 2, seed=17)       # Oxford at batch 2: a shape of the committed tuning table
    lp = gaussians(2, 3)
    sc = m.encode_aerial(s)
    logits, _, ori = m(g, s)[:3]
    _, post = m.track_update(g, s, lp)
    m.track_update_cached(g, sc, lp)
    gen = lib.ccvpe_tuning_generation(m._handle)

    def count(fn):
        torch.cuda.synchronize()
        n0 = lib.ccvpe_launch_count()
        fn()
        torch.cuda.synchronize()
        return int(lib.ccvpe_launch_count() - n0)

    for lm in (False, True):
        own = lambda: m.belief_credible(post, LEVELS, level_map=lm)
        pairs = [(lambda: m.localize_credible(g, s, LEVELS, lp, level_map=lm), lambda: m.track_update(g, s, lp)),
                 (lambda: m.localize_credible(g, s, LEVELS, level_map=lm, posterior=True), lambda: m.track_update(g, s)),
                 (lambda: m.localize_credible_cached(g, sc, LEVELS, lp, level_map=lm), lambda: m.track_update_cached(g, sc, lp)),
                 (lambda: m.localize_credible_cached(g, sc, LEVELS, lp, level_map=lm, tile_index=[1, 0]),
                  lambda: m.track_update_cached(g, sc, lp, tile_index=[1, 0])),
                 (lambda: m.postprocess_credible(logits, ori, LEVELS, lp, level_map=lm), lambda: m.track_update_logits(logits, ori, lp))]
        own()
        n_own = count(own)
        assert n_own == (5 if lm else 4)
        for a, b in pairs:
            a(); b()                      # plans and lazy kernel attributes exist before anything is counted
            na, nb = count(a), count(b)
            assert na == nb + n_own and nb > 0, (lm, na, nb, n_own)
    assert lib.ccvpe_tuning_generation(m._handle) == gen      # the credible plans took every tile from the table


# ---- 6. the trackers -------------------------------------------------------------------------------------------------------------

def test_trackers_append_the_cred_of_their_belief():
    m = make("oxford")
    F = 6
    g, s = inputs("oxford", F, seed=23)             # the six frames of tests/test_summary_gpu.py's tracker test
    sc = m.encode_aerial(s[:2])
    origins = np.array([[800, 400], [1200, 400]])
    tile = [0, 0, 0, 1, 1, 1]
    motion = np.array([61.0, -9.5])
    taps = aerial.gaussian_taps(3.0, 9)
    floor = 1e-7
    levels = (0.5, 0.9)
    plain, with_cred = aerial.Tracker(), aerial.Tracker()
    for k in range(F):
        gk, tk = g[k:k + 1], [tile[k]]
        rows = plain.step(m, gk, sc, tk, origins, motion, taps, floor)
        assert isinstance(rows, torch.Tensor)
        rows2, cred = with_cred.step(m, gk, sc, tk, origins, motion, taps, floor, credible_levels=levels)
        eq(rows2, rows)
        eq(with_cred.belief, plain.belief)
        assert cred.shape == (1, 10)
        eq_bits(cred, m.belief_credible(plain.belief, levels))
        assert 0.5 <= cred[0, 6].item() and 0.9 <= cred[0, 9].item() and cred[0, 5].item() <= cred[0, 8].item()
    # the affine tracker takes the same argument
    a, b = aerial.AffineTracker(), aerial.AffineTracker()
    ident = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    for k in range(2):
        rows = a.step(m, g[k:k + 1], None, ident, taps, floor, cache=sc, tile_index=[tile[k]])
        rows2, summ, cred = b.step(m, g[k:k + 1], None, ident, taps, floor, summary_radius=8, cache=sc, tile_index=[tile[k]],
                                   credible_levels=levels)
        eq(rows2, rows)
        eq(b.belief, a.belief)
        assert summ.shape == (1, 16)
        eq_bits(cred, m.belief_credible(a.belief, levels))
