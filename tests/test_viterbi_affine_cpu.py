"""The MAP trajectory behind an affine predict without a GPU: the C entry points and every refusal of
ccvpe_track_viterbi_affine and ccvpe_track_viterbi_back_affine (all made before the handle is used), the argument-check order of the
three Python functions, viterbi.map_path_affine against a fake model, the float64 definition tests/viterbi_affine_ref.py against a
dense Viterbi over all states of a small grid, the augmented link weight against the exact transition, the float32 restatement against
tests/viterbi_ref.py's at integer translations, the turning stream of tests/track_affine_ref.py started on a frame the distractor
wins, a turning stream that relocalises once, and a zero belief in the middle of a stream."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, smooth, viterbi
from tests import smooth_affine_ref, track_affine_ref, track_ref, viterbi_affine_ref as vref, viterbi_ref
from tests.test_viterbi_cpu import _buffers, _msg, model

EINVAL = -1
N = 512 * 512


# ---- C entry points --------------------------------------------------------------------------------------------------------

def test_entry_points_are_exported_and_bound(built_library):
    lib = C.CDLL(built_library)
    for n in ("ccvpe_track_viterbi_affine", "ccvpe_track_viterbi_back_affine"):
        assert hasattr(lib, n)
        assert n in {s for s, _, _ in _lib.SYMBOLS}
    assert callable(viterbi.track_viterbi_affine) and callable(viterbi.track_viterbi_back_affine) and callable(viterbi.map_path_affine)


def test_step_arguments_are_checked_before_the_handle(built_library):
    lib = _lib.load()
    bufs, (bel, bp, sp, ps, mt, tp, fl, out, st, wk) = _buffers(10)

    def call(belief=bel, belief_prev=bp, score_prev=sp, prev_stats=ps, batch=2, matrix=mt, taps=tp, stride=0, radius=3, floor=fl, score=out,
             stats=st, work=wk):
        return lib.ccvpe_track_viterbi_affine(None, belief, belief_prev, score_prev, prev_stats, batch, matrix, taps, stride, radius, floor,
                                              score, stats, work, None)

    first = dict(belief_prev=None, score_prev=None, prev_stats=None, matrix=None)
    for kw, word in ((dict(belief=None), "belief"), (dict(taps=None), "taps"), (dict(floor=None), "floor"), (dict(score=None), "score"),
                     (dict(stats=None), "stats"), (dict(work=None), "work")):
        assert call(**kw) == EINVAL and "null " + word in _msg(lib), (kw, _msg(lib))
    for kw, word in ((dict(belief=None), "belief"), (dict(score=None), "score"), (dict(stats=None), "stats"), (dict(work=None), "work")):
        assert call(**first, **kw) == EINVAL and "null " + word in _msg(lib), (kw, _msg(lib))
    names = list(first)
    for mask in range(1, 15):                                       # every proper subset of the four first-frame pointers
        kw = {n: None for i, n in enumerate(names) if mask >> i & 1}
        assert call(**kw) == EINVAL and "all null" in _msg(lib) and "matrix" in _msg(lib), (kw, _msg(lib))
    for bad in (-1, 33, 1000):
        assert call(radius=bad) == EINVAL and "radius" in _msg(lib), (bad, _msg(lib))
    for bad in (1, 3, 5, -4):
        assert call(stride=bad) == EINVAL and "taps_stride" in _msg(lib), (bad, _msg(lib))
    for bad in (0, -1, 4097):
        assert call(batch=bad) == EINVAL and "batch" in _msg(lib), (bad, _msg(lib))
        assert call(**first, batch=bad) == EINVAL and "batch" in _msg(lib), (bad, _msg(lib))
    for kw in (dict(score=bel), dict(score=bp), dict(score=sp), dict(score=ps), dict(score=wk), dict(score=st), dict(stats=wk), dict(stats=bel),
               dict(stats=bp), dict(stats=sp), dict(stats=ps)):
        assert call(**kw) == EINVAL and "alias" in _msg(lib), (kw, _msg(lib))
    assert call(**first, score=bel) == EINVAL and "alias" in _msg(lib)
    for name in ("belief", "belief_prev", "score_prev", "score", "work"):
        assert call(**{name: C.c_void_p(C.addressof(bufs[0]) + 64 + 4)}) == EINVAL and "aligned" in _msg(lib), (name, _msg(lib))
    for kw in (dict(), dict(radius=0), dict(radius=32), dict(stride=4), dict(batch=4096), dict(batch=1), first,
               dict(**first, taps=None, floor=None, radius=-7, stride=99)):
        assert call(**kw) == EINVAL and "null handle" in _msg(lib), (kw, _msg(lib))


def test_back_arguments_are_checked_before_the_handle(built_library):
    lib = _lib.load()
    bufs, (sp, ps, cell, mt, tp, fl, back) = _buffers(7)

    def call(score_prev=sp, prev_stats=ps, cell=cell, batch=2, matrix=mt, taps=tp, stride=0, radius=3, floor=fl, back=back):
        return lib.ccvpe_track_viterbi_back_affine(None, score_prev, prev_stats, cell, batch, matrix, taps, stride, radius, floor, back, None)

    for kw, word in ((dict(score_prev=None), "score_prev"), (dict(prev_stats=None), "prev_stats"), (dict(cell=None), "cell"),
                     (dict(matrix=None), "matrix"), (dict(taps=None), "taps"), (dict(floor=None), "floor"), (dict(back=None), "back")):
        assert call(**kw) == EINVAL and "null " + word in _msg(lib), (kw, _msg(lib))
    for bad in (-1, 33):
        assert call(radius=bad) == EINVAL and "radius" in _msg(lib), (bad, _msg(lib))
    for bad in (1, 3, -4):
        assert call(stride=bad) == EINVAL and "taps_stride" in _msg(lib), (bad, _msg(lib))
    for bad in (0, -1, 4097):
        assert call(batch=bad) == EINVAL and "batch" in _msg(lib), (bad, _msg(lib))
    for kw in (dict(back=sp), dict(back=ps), dict(back=cell)):
        assert call(**kw) == EINVAL and "alias" in _msg(lib), (kw, _msg(lib))
    assert call(score_prev=C.c_void_p(C.addressof(bufs[0]) + 64 + 4)) == EINVAL and "aligned" in _msg(lib)
    for kw in (dict(), dict(radius=0), dict(radius=32), dict(stride=4), dict(batch=4096)):
        assert call(**kw) == EINVAL and "null handle" in _msg(lib), (kw, _msg(lib))


# ---- the Python functions: the order of their checks -------------------------------------------------------------------------------

BEL, BEL_BAD = torch.zeros(2, 512, 512), torch.zeros(2, 512, 511)
ST, CELL = torch.zeros(2, 4), torch.zeros(2, dtype=torch.int32)
TAPS, TAPS_BAD, TAPS_LONG = np.ones(4, np.float32), np.ones((3, 4), np.float32), np.ones(34, np.float32)
MAT, MAT_BAD, MAT_INF = np.array([1.0, 0, 0, 0, 1, 0]), np.zeros((3, 6)), np.array([1.0, 0, np.inf, 0, 1, 0])
MAT_FAR = np.array([0.1, 0, 0, 0, 0.1, 0])          # beyond the smoother's reach (half extents 10), and singular: neither is refused here
R, V = RuntimeError, ValueError
ta, tb = viterbi.track_viterbi_affine, viterbi.track_viterbi_back_affine

CASES = [
    ("T>S", 1, lambda m: ta(m, BEL_BAD, BEL, BEL, ST, MAT, TAPS, 0.0), R, r"call \.eval\(\) first$"),
    ("S>mix", 0, lambda m: ta(m, BEL_BAD, BEL, None, ST, MAT, TAPS, 0.0), V, r"belief must be \[B,512,512\] or \[B,1,512,512\], got \(2, 512, 511\)"),
    ("mix>prev", 0, lambda m: ta(m, BEL, BEL_BAD, None, ST, MAT, TAPS, 0.0), V, r"prev_stats and matrix go together"),
    ("mix(matrix)", 0, lambda m: ta(m, BEL, matrix=MAT), V, r"go together"),
    ("prev>score", 0, lambda m: ta(m, BEL, BEL_BAD, BEL_BAD, ST, MAT, TAPS, 0.0), V, r"belief_prev must be \[B,512,512\] or \[B,1,512,512\], got \(2, 512, 511\)"),
    ("score(count)>stats", 0, lambda m: ta(m, BEL, BEL, torch.zeros(3, 512, 512), ST[:1], MAT, TAPS, 0.0), V, r"score_prev holds 3 maps, belief 2"),
    ("stats>matrix", 0, lambda m: ta(m, BEL, BEL, BEL, ST[:1], MAT_BAD, TAPS, 0.0), V, r"prev_stats must be a float32 tensor \[2, 4\]"),
    ("taps(none)>matrix", 0, lambda m: ta(m, BEL, BEL, BEL, ST, MAT_BAD), V, r"taps and floor of the predict call are needed"),
    ("matrix(shape)>taps", 0, lambda m: ta(m, BEL, BEL, BEL, ST, MAT_BAD, TAPS_BAD, 0.0), V, r"matrix must be \[6\] or \[2, 6\], got \(3, 6\)"),
    ("matrix(finite)>taps", 0, lambda m: ta(m, BEL, BEL, BEL, ST, MAT_INF, TAPS_BAD, 0.0), V, r"matrix must be finite"),
    ("taps>floor", 0, lambda m: ta(m, BEL, BEL, BEL, ST, MAT, TAPS_BAD, -1.0), V, r"taps must be \[radius\+1\] or \[2, radius\+1\], got \(3, 4\)"),
    ("radius>floor", 0, lambda m: ta(m, BEL, BEL, BEL, ST, MAT, TAPS_LONG, -1.0), V, r"taps give radius 33, must be in 0\.\.32$"),
    ("floor>D", 0, lambda m: ta(m, BEL, BEL, BEL, ST, MAT, TAPS, -1.0), V, r"floor must be >= 0"),
    ("ends", 0, lambda m: ta(m, BEL, BEL, BEL, ST, MAT, TAPS, 0.0), V, r"belief must be a cuda tensor, not a cpu tensor"),
    ("no reach rule", 0, lambda m: ta(m, BEL, BEL, BEL, ST, MAT_FAR, TAPS, 0.0), V, r"belief must be a cuda tensor, not a cpu tensor"),
    ("first ends", 0, lambda m: ta(m, BEL), V, r"belief must be a cuda tensor, not a cpu tensor"),
    ("back T>S", 1, lambda m: tb(m, BEL_BAD, ST, CELL, MAT, TAPS, 0.0), R, r"call \.eval\(\) first$"),
    ("back S>stats", 0, lambda m: tb(m, BEL_BAD, ST[:1], CELL, MAT, TAPS, 0.0), V, r"score_prev must be \[B,512,512\] or \[B,1,512,512\], got \(2, 512, 511\)"),
    ("back stats>cell", 0, lambda m: tb(m, BEL, ST[:1], CELL.long(), MAT, TAPS, 0.0), V, r"prev_stats must be a float32 tensor \[2, 4\]"),
    ("back cell>matrix", 0, lambda m: tb(m, BEL, ST, CELL.long(), MAT_BAD, TAPS, 0.0), V, r"cell must be an int32 tensor \[2\]"),
    ("back matrix>taps", 0, lambda m: tb(m, BEL, ST, CELL, MAT_BAD, TAPS_BAD, 0.0), V, r"matrix must be \[6\] or \[2, 6\], got \(3, 6\)"),
    ("back matrix(finite)", 0, lambda m: tb(m, BEL, ST, CELL, MAT_INF, TAPS_BAD, 0.0), V, r"matrix must be finite"),
    ("back taps>floor", 0, lambda m: tb(m, BEL, ST, CELL, MAT, TAPS_BAD, -1.0), V, r"taps must be \[radius\+1\] or \[2, radius\+1\], got \(3, 4\)"),
    ("back floor>D", 0, lambda m: tb(m, BEL, ST, CELL, MAT, TAPS, -1.0), V, r"floor must be >= 0"),
    ("back ends", 0, lambda m: tb(m, BEL, ST, CELL, MAT_FAR, TAPS, 0.0), V, r"score_prev must be a cuda tensor, not a cpu tensor"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_error_precedence(case):
    _, training, call, exc, message = case
    with pytest.raises(exc, match=message):
        call(model(bool(training)))


def test_the_smoother_still_refuses_what_it_refused():
    """smooth.track_smooth_affine shares the matrix check and keeps its reach rule behind it"""
    m = model()
    with pytest.raises(V, match=r"matrix must be \[6\] or \[2, 6\], got \(3, 6\)"):
        smooth.track_smooth_affine(m, BEL, BEL, MAT_BAD, TAPS_BAD, 0.0)
    with pytest.raises(V, match=r"matrix must be finite"):
        smooth.track_smooth_affine(m, BEL, BEL, MAT_INF, TAPS_BAD, 0.0)
    with pytest.raises(V, match=r"matrix 0 is beyond the smoother's reach"):
        smooth.track_smooth_affine(m, BEL, BEL, MAT_FAR, TAPS_BAD, 0.0)


# ---- map_path_affine against a fake model ---------------------------------------------------------------------------------------------

def test_map_path_affine_makes_the_calls_in_order(monkeypatch):
    T, B = 4, 2
    log = [(torch.full((B, 512, 512), float(t + 1)), None if t == 0 else np.full((B, 6), float(t)), np.ones(3, np.float32) * t, 1e-7 * t)
           for t in range(T)]
    calls = []

    def fake_step(model, belief, belief_prev=None, score_prev=None, prev_stats=None, matrix=None, taps=None, floor=None, out=None):
        t = int(belief[0, 0, 0]) - 1
        calls.append(("step", t, None if belief_prev is None else int(belief_prev[0, 0, 0]) - 1,
                      None if score_prev is None else float(score_prev[0, 0, 0]), None if prev_stats is None else float(prev_stats[0, 2]),
                      None if matrix is None else float(np.asarray(matrix)[0, 0]), None if taps is None else float(taps[0]), floor))
        st = torch.tensor([[100.0 + t, 1.5, float(t), 0.0]] * B)
        return torch.full((B, 512, 512), 10.0 + t), st

    def fake_back(model, score_prev, prev_stats, cell, matrix, taps, floor):
        assert cell.dtype == torch.int32 and tuple(cell.shape) == (B,)
        calls.append(("back", float(score_prev[0, 0, 0]), float(prev_stats[0, 2]), cell.tolist(), float(np.asarray(matrix)[0, 0]), float(taps[0]), floor))
        return torch.tensor([[int(cell[0]) - 50, viterbi.LINK_MOVE], [int(cell[1]) - 60, viterbi.LINK_JUMP]], dtype=torch.int32)

    def never(*a, **kw):
        raise AssertionError("the translation calls are not map_path_affine's")

    monkeypatch.setattr(viterbi, "track_viterbi_affine", fake_step)
    monkeypatch.setattr(viterbi, "track_viterbi_back_affine", fake_back)
    monkeypatch.setattr(viterbi, "track_viterbi", never)
    monkeypatch.setattr(viterbi, "track_viterbi_back", never)
    cells, links, stats, scores = viterbi.map_path_affine(object(), log)
    assert calls[:T] == [("step", 0, None, None, None, None, None, None)] + \
        [("step", t, t - 1, 10.0 + t - 1, float(t - 1), float(t), float(t), 1e-7 * t) for t in range(1, T)]
    assert calls[T:] == [("back", 10.0 + t - 1, float(t - 1), [103 - 50 * (T - 1 - t), 103 - 60 * (T - 1 - t)], float(t), float(t), 1e-7 * t)
                         for t in range(T - 1, 0, -1)]
    assert cells.dtype == torch.int32 and links.dtype == torch.int32
    assert cells.tolist() == [[103 - 50 * (T - 1 - t), 103 - 60 * (T - 1 - t)] for t in range(T)]
    assert links.tolist() == [[viterbi.LINK_START] * B] + [[viterbi.LINK_MOVE, viterbi.LINK_JUMP]] * (T - 1)
    assert tuple(stats.shape) == (T, B, 4) and len(scores) == T and [float(s[0, 0, 0]) for s in scores] == [10.0, 11.0, 12.0, 13.0]
    with pytest.raises(ValueError, match="empty"):
        viterbi.map_path_affine(object(), [])
    with pytest.raises(ValueError, match="no matrix"):
        viterbi.map_path_affine(object(), [log[0], log[0]])


# ---- the definition against a dense Viterbi; the augmented weight against the exact one ------------------------------------------------

HMM_HW, HMM_T = 12, 5
HMM_C = ((HMM_HW - 1) / 2.0,) * 2
HMM_MATS = smooth_affine_ref.quantise(np.stack([
    aerial.rigid_matrix(7.0, [1.3, -0.4], centre=HMM_C), aerial.rigid_matrix(-4.0, [-0.7, 1.6], centre=HMM_C),
    aerial.rigid_matrix(3.0, [0.25, 0.9], 0.8, centre=HMM_C), np.array([1.0, 0.0, -2.0, 0.0, 1.0, 1.0])]))
HMM_TAPS = aerial.gaussian_taps(0.9, 2)
HMM_FLOOR = np.float32(1e-3)


def test_definition_is_the_dense_viterbi_of_the_augmented_model():
    """5 frames on a 12 x 12 grid: the float64 definition, run on the exact dense filter's beliefs, walks the path of the textbook
    recursion over all 144 states with transition max(T_aug, floor) - cells and link kinds."""
    n = HMM_HW * HMM_HW
    for seed in (5, 6, 7):
        like = np.random.default_rng(seed).uniform(0.05, 1.0, size=(HMM_T, n)) ** 4
        alpha, _ = smooth_affine_ref.dense_forward_backward(like, HMM_MATS, HMM_TAPS, float(HMM_FLOOR), HMM_HW)
        want_cells, want_kinds = vref.dense_viterbi(like, HMM_MATS, HMM_TAPS, float(HMM_FLOOR), HMM_HW)
        cells, links, stats, _ = vref.sweep([a.reshape(HMM_HW, HMM_HW) for a in alpha], [None] + list(HMM_MATS), HMM_TAPS, HMM_FLOOR, HMM_HW)
        assert cells.tolist() == want_cells.tolist(), (seed, cells, want_cells)
        assert links.tolist() == want_kinds.tolist(), (seed, links, want_kinds)
        assert stats[0, 3] == 1 and not stats[1:, 3].any() and ((stats[:, 1] >= 1) & (stats[:, 1] < 2)).all()


def test_augmented_weight_brackets_the_exact_transition():
    """T_aug <= T <= ceil(2 hx) ceil(2 hy) T_aug against the exact dense transition, with equality at the integer translation; the
    augmented weight is positive wherever the exact one is."""
    mats = list(HMM_MATS) + [smooth_affine_ref.quantise(aerial.rigid_matrix(45.0, [0.3, 0.2], centre=HMM_C))]
    for k, mat in enumerate(mats):
        exact = smooth_affine_ref.dense_kernel(mat, HMM_TAPS, HMM_HW)
        aug = vref.dense_augmented(mat, HMM_TAPS, HMM_HW)
        hx, hy = smooth.affine_reach(mat)
        count = np.ceil(2 * hx) * np.ceil(2 * hy)
        assert (aug <= exact * (1 + 1e-12)).all(), k
        assert (exact <= count * aug * (1 + 1e-12)).all(), (k, count, float((exact / np.where(aug > 0, aug, np.inf)).max()))
        assert ((aug > 0) == (exact > 0)).all(), k
        if k == 3:
            np.testing.assert_allclose(aug, exact, rtol=1e-14, atol=0)
        else:
            assert (exact > aug * (1 + 1e-9)).any(), k


# ---- integer translations: viterbi_ref's bits --------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [0, 1, 6])
def test_integer_translations_give_the_float32_bits_of_the_translation_form(r):
    hw = 40
    rng = np.random.default_rng(40 + r)
    taps = aerial.gaussian_taps(0.8 + 0.3 * r, r)
    floor = np.float32(1e-4)
    prev = rng.uniform(0.0, 1.0, size=(hw, hw)).astype(np.float32) ** 3
    prev /= prev.sum()
    vp = viterbi_ref.step(prev[None], hw=hw, dtype=np.float32)
    bel = rng.uniform(0.0, 1.0, size=(1, hw, hw)).astype(np.float32) ** 3
    for dx, dy in ((0, 0), (3, -2), (-7, 11), (45, 1)):                     # the last one leaves the grid
        shift = np.float32([[dx, dy]])
        mat = np.array([1.0, 0.0, -dx, 0.0, 1.0, -dy])
        want = viterbi_ref.step(bel, prev[None], vp["v"], vp["stats"], shift, taps, floor, hw, np.float32)
        got = vref.step(bel, prev[None], vp["v"], vp["stats"], mat, taps, floor, hw, np.float32)
        np.testing.assert_array_equal(vref.max_passes(vp["v"][0], mat, taps, hw, np.float32), viterbi_ref.max_passes(vp["v"][0], shift[0], taps, hw, np.float32))
        for key in ("v", "w", "win", "jump", "stats"):
            np.testing.assert_array_equal(got[key], want[key], err_msg=f"{key} at {(dx, dy)}")
        for cell in [int(want["stats"][0, 0]), 0, hw * hw - 1, -1, hw * hw] + rng.integers(0, hw * hw, size=12).tolist():
            assert vref.back(vp["v"][0], vp["stats"][0], cell, mat, taps, floor, hw, np.float32) == \
                viterbi_ref.back(vp["v"][0], vp["stats"][0], cell, shift[0], taps, floor, hw, np.float32), (cell, dx, dy)


# ---- streams ---------------------------------------------------------------------------------------------------------------------

def test_turning_stream_path_stays_on_the_truth():
    """Frames 2 .. 11 of tests/track_affine_ref's turning stream in float64.  The filter has no prior for frame 2, a SEQ_STRONG frame: its
    argmax is the distractor, more than 250 px off.  The path is within 1 px of the truth in every frame, every link is a MOVE, and from
    frame 4 on the best score on the distractor is below 1e-3 of the peak, so a float32 rounding cannot flip a cell."""
    ref = track_affine_ref
    frames, beliefs, _, cells, links, scores, _ = vref.turning_path()
    assert frames == list(range(2, ref.SEQ_FRAMES)) and len(frames) == 10
    assert track_ref.pixel_distance(int(np.argmax(beliefs[0])), ref.sequence_truth(frames[0])) > 250.0
    worst = max(track_ref.pixel_distance(int(cells[t]), ref.sequence_truth(k)) for t, k in enumerate(frames))
    dx, dy = (int(v) for v in ref.SEQ_DISTRACTOR)
    ratios = [float(scores[t][dy - 8:dy + 9, dx - 8:dx + 9].max() / scores[t].max()) for t in range(len(frames))]
    print(f"worst distance {worst:.3f} px, distractor / peak per frame {['%.2g' % v for v in ratios]}")
    assert worst <= 1.0
    assert links.tolist() == [vref.START] + [vref.MOVE] * (len(frames) - 1)
    for t, k in enumerate(frames):
        if k >= 4:
            assert ratios[t] < 1e-3, (k, ratios[t])


def test_relocalising_turning_stream_jumps_once():
    truth, _, _, cells, links, _, _ = vref.reloc_path()
    for t in range(vref.RELOC_T):
        assert track_ref.pixel_distance(int(cells[t]), truth[t]) <= 1.0, (t, cells[t], truth[t])
    want = [vref.START] + [vref.MOVE] * (vref.RELOC_T - 1)
    want[vref.RELOC_AT] = vref.JUMP
    assert links.tolist() == want


def test_zero_belief_mid_stream_ends_one_segment_and_starts_the_next():
    """As in tests/test_viterbi_cpu.py, through a frame that turns by 5 degrees per link: the zero frame has cell -1 and START on both
    sides, and each segment's cells are those of the segment run alone."""
    hw, T, z = 64, 7, 3
    taps, floor = aerial.gaussian_taps(1.0, 3), np.float32(1e-6)
    c = np.array([31.5, 31.5])
    rot = lambda k: track_affine_ref._rot(k * 5.0 / track_affine_ref.SEQ_TURN_DEG)
    truth = [c + rot(k) @ (np.array([14.0 + 3.3 * k, 24.0 + 1.6 * k]) - c) for k in range(T)]
    mats = [None] + [smooth_affine_ref.quantise(aerial.rigid_matrix(5.0, rot(k) @ np.array([3.3, 1.6]), centre=tuple(c))) for k in range(1, T)]
    logits = [viterbi_ref.peak_logits(xy, hw) for xy in truth]

    def filt(ks):
        out = []
        for k in ks:
            lg = logits[k].astype(np.float64)
            if out:
                lg = lg + np.log(smooth_affine_ref.predict_c64(out[-1], mats[k], taps, hw)[0].reshape(-1) + float(floor))
            e = np.exp(lg - lg.max())
            out.append((e / e.sum()).reshape(hw, hw))
        return out

    beliefs = filt(range(z)) + [np.zeros((hw, hw))] + filt(range(z + 1, T))
    cells, links, stats, _ = vref.sweep(beliefs, mats, taps, floor, hw)
    assert cells[z] == -1 and links[z] == vref.START and links[z + 1] == vref.START
    assert stats[z, 0] == -1 and np.isnan(stats[z, 1]) and stats[z, 3] == 0 and stats[z + 1, 3] == 1
    head, head_links, _, _ = vref.sweep(beliefs[:z], mats[:z], taps, floor, hw)
    tail, tail_links, _, _ = vref.sweep(beliefs[z + 1:], [None] + mats[z + 2:], taps, floor, hw)
    assert cells[:z].tolist() == head.tolist() and cells[z + 1:].tolist() == tail.tolist()
    assert links[:z].tolist() == head_links.tolist() and links[z + 1:].tolist() == tail_links.tolist()
    for t in list(range(z)) + list(range(z + 1, T)):
        assert track_ref.pixel_distance(int(cells[t]), tuple(truth[t]), hw) <= 1.0, t
