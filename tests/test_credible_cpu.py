"""Credible regions without a GPU: the sorting restatement tests/credible_ref.py against the defining property of the
region, computed without sorting, on every crafted map and level; the probe rule; the names in the header, the library and
ccvpe_amd._lib; and every refusal of the four entry points, which are checked before the handle is used and so need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ccvpe_amd import _lib, aerial
from tests import credible_ref as cr
from tests import summary_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ccvpe_belief_credible", "ccvpe_postprocess_credible", "ccvpe_localize_credible", "ccvpe_localize_credible_cached_indexed")
MAPS = sr.crafted_maps()
EINVAL = -1


def probes_of(h):
    """three cells of a map: its peak, a cell of its smallest value (a zero cell where there is one), and one in between"""
    f = h.reshape(-1)
    return [int(np.argmax(f)), int(np.argmin(f)), int(np.argsort(f, kind="stable")[f.size // 2])]


@pytest.mark.parametrize("name", sorted(MAPS))
def test_restatement_has_the_defining_property(name):
    h = MAPS[name]
    k, q = cr.keys_masses(h)
    Q = int(q.sum(dtype=np.uint64))
    assert Q > 0
    cells = probes_of(h)
    rows = [cr.credible(h, cr.LEVELS, probe=c, level_map=True) for c in cells]
    row, lm = rows[0]
    assert row[0] == np.float32(Q * 2.0 ** -44) and row[1] == int((k != 0).sum())
    inside = np.zeros(cr.N, np.int64)
    for j, p in enumerate(cr.LEVELS):
        T = cr.threshold(p, Q)
        assert 1 <= T <= Q
        kstar = int(cr.bits(row[4 + 3 * j:5 + 3 * j])[0])
        assert kstar != 0 and (k == kstar).any(), "k* is a key present in the map"
        G = int(q[k >= kstar].sum(dtype=np.uint64))
        assert G >= T, "the region holds the share"
        assert int(q[k > kstar].sum(dtype=np.uint64)) < T, "and no smaller union of whole value classes does"
        assert row[5 + 3 * j] == int((k >= kstar).sum())
        assert row[6 + 3 * j] == np.float32(np.float64(G) / np.float64(Q))
        inside += k >= kstar
        # the probe rule: the cell lies in the region exactly when the mass strictly above it is below T
        for c, (prow, _) in zip(cells, rows):
            above = int(q[k > k[c]].sum(dtype=np.uint64))
            assert (above < T) == bool(k[c] >= kstar), (name, p, c)
            assert prow[2] == np.float32(np.float64(above) / np.float64(Q)) and prow[3] == int((k > k[c]).sum())
            assert (cr.bits(prow[4:]) == cr.bits(row[4:])).all(), "the probe changes no level column"
    assert (lm == inside).all()
    if name == "uniform":          # one value class holds everything: every level's region is the whole map
        assert (row[5::3] == cr.N).all() and (lm == len(cr.LEVELS)).all()
    if name == "two_deltas":       # the exact 0.5 boundary: both cells tie, so no level splits them
        assert (row[5::3] == 2).all()


def test_restatement_of_the_special_maps():
    levels = (0.5, 1.0)
    row, lm = cr.credible(np.zeros((512, 512), np.float32), levels, probe=7, level_map=True)
    assert row[0] == 0 and row[1] == 0 and np.isnan(row[2]) and row[3] == 0
    assert np.isnan(row[[4, 6, 7, 9]]).all() and (row[[5, 8]] == 0).all() and not lm.any()
    tiny = np.full((512, 512), np.float32(2.0 ** -50))
    row, lm = cr.credible(tiny, levels, probe=-1, level_map=True)
    assert row[0] == 0 and row[1] == cr.N and np.isnan(row[2:4]).all() and np.isnan(row[[4, 6]]).all() and not lm.any()   # keys, no mass
    odd = MAPS["random"].copy()
    odd[10, 20] = np.nan
    odd[400, 17] = 2.0
    odd[0, 0] = np.inf
    k, q = cr.keys_masses(odd)
    assert k[10 * 512 + 20] == 0 and q[400 * 512 + 17] == 2 ** 44 and q[0] == 2 ** 44 and k[0] == 0x7F800000
    row, _ = cr.credible(odd, (1e-6,), probe=400 * 512 + 17)
    assert row[3] == 1 and np.isinf(row[4]) and row[5] == 1          # +inf is a value: it orders above 2.0 and weighs 1


def test_python_helpers():
    h = MAPS["two_deltas"]
    cells = probes_of(h)
    rows = np.stack([cr.credible(h, cr.LEVELS, probe=c)[0] for c in cells])
    k, _ = cr.keys_masses(h)
    want = np.array([[bool(k[c] >= cr.bits(rows[0, 4 + 3 * j:5 + 3 * j])[0]) for j in range(len(cr.LEVELS))] for c in cells])
    assert (aerial.credible_contains(rows, cr.LEVELS) == want).all()
    assert not aerial.credible_contains(cr.credible(h, (0.5,))[0], (0.5,)).any()          # no probe: NaN columns
    m = aerial.credible_to_metres(rows, 0.5)
    assert (m[:, 5::3] == rows[:, 5::3] * 0.25).all()
    keep = np.ones(rows.shape[1], bool)
    keep[5::3] = False
    assert (cr.bits(m[:, keep]) == cr.bits(rows[:, keep])).all()
    assert len(aerial.CREDIBLE_HEAD_FIELDS) == 4 and len(aerial.CREDIBLE_LEVEL_FIELDS) == 3
    with pytest.raises(ValueError):
        aerial.credible_to_metres(rows[:, :6], 1.0)


def test_names_agree_in_header_library_and_bindings(built_library):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ccvpe.h")).read(), flags=re.S)
    lib = C.CDLL(built_library)
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    for n in NAMES:
        m = re.search(r"\bint %s\s*\(([^;]*)\);" % n, text)
        assert m, f"{n} is not declared in include/ccvpe.h"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in bound and len(bound[n]) == len(m.group(1).split(",")), f"{n}: ccvpe_amd._lib binds another argument list"
    assert re.search(r"#define\s+CCVPE_CREDIBLE_MAX_LEVELS\s+8\b", text)


def test_refusals_come_before_the_handle(built_library):
    """every refusal returns CCVPE_EINVAL and names its argument; the handle is null throughout and the fake device pointers are
    never dereferenced"""
    lib = _lib.load()
    P = [C.c_void_p(0x1000 * (i + 1)) for i in range(12)]
    bel, lg, ori, prior, probe, rows, cred, lmap, post, grd, sat, cache = P
    levels = (C.c_float * 3)(0.5, 0.9, 1.0)
    n = 512 * 512
    tiles = (C.c_int32 * 2)(0, 1)

    def belief(**kw):
        a = dict(belief=bel, batch=2, levels=levels, n_levels=3, probe=probe, cred=cred, level_map=lmap)
        a.update(kw)
        return lib.ccvpe_belief_credible(None, a["belief"], a["batch"], a["levels"], a["n_levels"], a["probe"], a["cred"], a["level_map"], None)

    def logits(**kw):
        a = dict(logits=lg, ori=ori, batch=2, log_prior=prior, prior_stride=n, levels=levels, n_levels=3, probe=probe, rows=rows, cred=cred,
                 level_map=lmap, posterior=post)
        a.update(kw)
        return lib.ccvpe_postprocess_credible(None, a["logits"], a["ori"], a["batch"], a["log_prior"], a["prior_stride"], a["levels"],
                                              a["n_levels"], a["probe"], a["rows"], a["cred"], a["level_map"], a["posterior"], None)

    def full(**kw):
        a = dict(grd=grd, sat=sat, batch=2, log_prior=prior, prior_stride=n, levels=levels, n_levels=3, probe=probe, rows=rows, cred=cred,
                 level_map=lmap, posterior=post)
        a.update(kw)
        return lib.ccvpe_localize_credible(None, a["grd"], 154, 231, a["sat"], a["batch"], a["log_prior"], a["prior_stride"], a["levels"],
                                           a["n_levels"], a["probe"], a["rows"], a["cred"], a["level_map"], a["posterior"], None)

    def cached(**kw):
        a = dict(grd=grd, cache=cache, n_tiles=2, tile_index=tiles, batch=2, log_prior=prior, prior_stride=n, levels=levels, n_levels=3,
                 probe=probe, rows=rows, cred=cred, level_map=lmap, posterior=post)
        a.update(kw)
        return lib.ccvpe_localize_credible_cached_indexed(None, a["grd"], 154, 231, a["cache"], a["n_tiles"], a["tile_index"], a["batch"],
                                                          a["log_prior"], a["prior_stride"], a["levels"], a["n_levels"], a["probe"],
                                                          a["rows"], a["cred"], a["level_map"], a["posterior"], None)

    def refused(rc, *words):
        msg = lib.ccvpe_last_error().decode()
        assert rc == EINVAL, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    # good arguments reach the handle check, and only that one
    for fn in (belief, logits, full, cached):
        refused(fn(), "null handle")
        refused(fn(probe=None, level_map=None), "null handle")
        # the levels
        refused(fn(levels=None), "levels")
        refused(fn(cred=None), "cred")
        refused(fn(n_levels=0), "n_levels", "0")
        refused(fn(n_levels=9), "n_levels", "9")
        for bad in (0.0, -0.5, 1.5, float("nan"), float("inf")):
            refused(fn(levels=(C.c_float * 3)(0.5, bad, 1.0)), "levels[1]", "%g" % bad)
        # aliasing of the two outputs
        refused(fn(level_map=cred), "level_map", "cred")
        refused(fn(cred=probe), "cred", "probe")
        refused(fn(level_map=probe), "level_map", "probe")
    # the stored-map form
    refused(belief(belief=None), "belief")
    refused(belief(batch=0), "batch")
    refused(belief(batch=4097), "batch", "4097")
    refused(belief(belief=C.c_void_p(0x1002)), "belief", "aligned")
    refused(belief(cred=bel), "cred", "belief")
    refused(belief(level_map=bel), "level_map", "belief")
    # the forms with rows
    for fn in (logits, full, cached):
        refused(fn(rows=None), "rows")
        refused(fn(prior_stride=5), "prior_stride")
        refused(fn(log_prior=None, prior_stride=5, posterior=None), "null handle")       # the stride is read only beside a prior
        refused(fn(posterior=None), "null handle")
        for other in ("log_prior", "rows", "posterior"):
            refused(fn(cred=a_ptr(other, prior, rows, post)), "cred", other)
            refused(fn(level_map=a_ptr(other, prior, rows, post)), "level_map", other)
        refused(fn(posterior=prior), "posterior", "log_prior")
    refused(logits(logits=None), "logits")
    refused(logits(ori=None), "ori")
    refused(logits(batch=0), "batch")
    refused(logits(batch=4097), "batch", "4097")
    refused(logits(cred=lg), "cred", "logits")
    refused(logits(level_map=ori), "level_map", "ori")
    refused(logits(posterior=lg), "posterior", "logits")
    refused(full(grd=None), "grd")
    refused(full(sat=None), "sat")
    refused(full(cred=sat), "cred", "sat")
    refused(cached(grd=None), "grd")
    refused(cached(cache=None), "cache")
    refused(cached(cred=cache), "cred", "cache")
    refused(cached(tile_index=(C.c_int32 * 2)(0, 2)), "tile_index[1]")
    refused(cached(tile_index=None, n_tiles=3), "n_tiles")


def a_ptr(name, prior, rows, post):
    return {"log_prior": prior, "rows": rows, "posterior": post}[name]
