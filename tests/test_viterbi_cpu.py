"""The MAP trajectory without a GPU: the C entry points and every refusal of ccvpe_track_viterbi and
ccvpe_track_viterbi_back (all made before the handle is used), the argument-check order of viterbi.track_viterbi and
viterbi.track_viterbi_back, the float64 definition tests/viterbi_ref.py against a dense Viterbi over all states of a small grid, the
crafted stream of tests/track_ref.py started on a frame the distractor wins, a stream that relocalises once, a zero belief in the
middle of a stream, and viterbi.map_path against a fake model."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models, viterbi
from tests import smooth_ref, track_ref, viterbi_ref

EINVAL = -1
N = 512 * 512


# ---- C entry points --------------------------------------------------------------------------------------------------------

def test_entry_points_are_exported_and_bound(built_library):
    lib = C.CDLL(built_library)
    for n in ("ccvpe_track_viterbi", "ccvpe_track_viterbi_back", "ccvpe_track_viterbi_work_bytes"):
        assert hasattr(lib, n)
        assert n in {s for s, _, _ in _lib.SYMBOLS}
    assert viterbi.VITERBI_FIELDS == ("index", "peak", "exponent", "restarted")
    assert (viterbi.LINK_MOVE, viterbi.LINK_JUMP, viterbi.LINK_START) == (0, 1, 2) == (viterbi_ref.MOVE, viterbi_ref.JUMP, viterbi_ref.START)
    assert callable(viterbi.track_viterbi) and callable(viterbi.track_viterbi_back) and callable(viterbi.map_path)


def test_work_bytes_cover_the_tile_pairs_only(built_library):
    lib = _lib.load()
    for batch in (1, 2, 3, 32, 4096):
        assert lib.ccvpe_track_viterbi_work_bytes(batch) == batch * 256 * 2 * 4
    assert lib.ccvpe_track_viterbi_work_bytes(0) == 0 and lib.ccvpe_track_viterbi_work_bytes(-3) == 0


def _buffers(k):
    bufs = [(C.c_float * 64)() for _ in range(k)]                     # (ctypes arrays of this size are 16-byte aligned)
    assert all(C.addressof(b) % 16 == 0 for b in bufs)
    return bufs, [C.cast(b, C.c_void_p) for b in bufs]


def _msg(lib):
    return (lib.ccvpe_last_error() or b"").decode()


def test_step_arguments_are_checked_before_the_handle(built_library):
    lib = _lib.load()
    bufs, (bel, bp, sp, ps, sh, tp, fl, out, st, wk) = _buffers(10)

    def call(belief=bel, belief_prev=bp, score_prev=sp, prev_stats=ps, batch=2, shift=sh, taps=tp, stride=0, radius=3, floor=fl, score=out,
             stats=st, work=wk):
        return lib.ccvpe_track_viterbi(None, belief, belief_prev, score_prev, prev_stats, batch, shift, taps, stride, radius, floor, score,
                                       stats, work, None)

    first = dict(belief_prev=None, score_prev=None, prev_stats=None, shift=None)
    for kw, word in ((dict(belief=None), "belief"), (dict(taps=None), "taps"), (dict(floor=None), "floor"), (dict(score=None), "score"),
                     (dict(stats=None), "stats"), (dict(work=None), "work")):
        assert call(**kw) == EINVAL and "null " + word in _msg(lib), (kw, _msg(lib))
    for kw, word in ((dict(belief=None), "belief"), (dict(score=None), "score"), (dict(stats=None), "stats"), (dict(work=None), "work")):
        assert call(**first, **kw) == EINVAL and "null " + word in _msg(lib), (kw, _msg(lib))
    # a mix of NULL and non-NULL among the four first-frame pointers: every proper subset
    names = list(first)
    for mask in range(1, 15):
        kw = {n: None for i, n in enumerate(names) if mask >> i & 1}
        assert call(**kw) == EINVAL and "all null" in _msg(lib), (kw, _msg(lib))
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
    # what is allowed reaches the handle: both forms (the first frame looks at no taps, stride, radius or floor), every radius, both strides
    for kw in (dict(), dict(radius=0), dict(radius=32), dict(stride=4), dict(batch=4096), dict(batch=1), first,
               dict(**first, taps=None, floor=None, radius=-7, stride=99)):
        assert call(**kw) == EINVAL and "null handle" in _msg(lib), (kw, _msg(lib))


def test_back_arguments_are_checked_before_the_handle(built_library):
    lib = _lib.load()
    bufs, (sp, ps, cell, sh, tp, fl, back) = _buffers(7)

    def call(score_prev=sp, prev_stats=ps, cell=cell, batch=2, shift=sh, taps=tp, stride=0, radius=3, floor=fl, back=back):
        return lib.ccvpe_track_viterbi_back(None, score_prev, prev_stats, cell, batch, shift, taps, stride, radius, floor, back, None)

    for kw, word in ((dict(score_prev=None), "score_prev"), (dict(prev_stats=None), "prev_stats"), (dict(cell=None), "cell"), (dict(shift=None), "shift"),
                     (dict(taps=None), "taps"), (dict(floor=None), "floor"), (dict(back=None), "back")):
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

_M = {}


def model(training=False):
    if training not in _M:
        m = models.CVM_OxfordRobotCar("cpu")
        _M[training] = m.train() if training else m.eval()
    return _M[training]


BEL, BEL_BAD = torch.zeros(2, 512, 512), torch.zeros(2, 512, 511)
ST, CELL = torch.zeros(2, 4), torch.zeros(2, dtype=torch.int32)
TAPS, TAPS_BAD, TAPS_LONG = np.ones(4, np.float32), np.ones((3, 4), np.float32), np.ones(34, np.float32)
SHIFT, SHIFT_BAD = np.zeros((2, 2)), np.zeros((3, 2))
R, V = RuntimeError, ValueError
tv, tb = viterbi.track_viterbi, viterbi.track_viterbi_back

# (id, training, call, exception, message): every call but the last of a function carries two faults of neighbouring check groups
CASES = [
    ("T>S", 1, lambda m: tv(m, BEL_BAD, BEL, BEL, ST, SHIFT, TAPS, 0.0), R, r"call \.eval\(\) first$"),
    ("S>mix", 0, lambda m: tv(m, BEL_BAD, BEL, None, ST, SHIFT, TAPS, 0.0), V, r"belief must be \[B,512,512\] or \[B,1,512,512\], got \(2, 512, 511\)"),
    ("mix>prev", 0, lambda m: tv(m, BEL, BEL_BAD, None, ST, SHIFT, TAPS, 0.0), V, r"go together"),
    ("mix(shift)", 0, lambda m: tv(m, BEL, shift_px=SHIFT), V, r"go together"),
    ("prev>score", 0, lambda m: tv(m, BEL, BEL_BAD, BEL_BAD, ST, SHIFT, TAPS, 0.0), V, r"belief_prev must be \[B,512,512\] or \[B,1,512,512\], got \(2, 512, 511\)"),
    ("score(count)>stats", 0, lambda m: tv(m, BEL, BEL, torch.zeros(3, 512, 512), ST[:1], SHIFT, TAPS, 0.0), V, r"score_prev holds 3 maps, belief 2"),
    ("stats>taps", 0, lambda m: tv(m, BEL, BEL, BEL, ST[:1], SHIFT, TAPS_BAD, 0.0), V, r"prev_stats must be a float32 tensor \[2, 4\]"),
    ("taps(none)", 0, lambda m: tv(m, BEL, BEL, BEL, ST, SHIFT), V, r"taps and floor of the predict call are needed"),
    ("taps>floor", 0, lambda m: tv(m, BEL, BEL, BEL, ST, SHIFT, TAPS_BAD, -1.0), V, r"taps must be \[radius\+1\] or \[2, radius\+1\], got \(3, 4\)"),
    ("radius>floor", 0, lambda m: tv(m, BEL, BEL, BEL, ST, SHIFT, TAPS_LONG, -1.0), V, r"taps give radius 33, must be in 0\.\.32$"),
    ("floor>shift", 0, lambda m: tv(m, BEL, BEL, BEL, ST, SHIFT_BAD, TAPS, -1.0), V, r"floor must be >= 0"),
    ("shift>D", 0, lambda m: tv(m, BEL, BEL, BEL, ST, SHIFT_BAD, TAPS, 0.0), V, r"shift_px must have shape \(2, 2\), got \(3, 2\)"),
    ("ends", 0, lambda m: tv(m, BEL, BEL, BEL, ST, SHIFT, TAPS, 0.0), V, r"belief must be a cuda tensor, not a cpu tensor"),
    ("first ends", 0, lambda m: tv(m, BEL), V, r"belief must be a cuda tensor, not a cpu tensor"),
    ("back T>S", 1, lambda m: tb(m, BEL_BAD, ST, CELL, SHIFT, TAPS, 0.0), R, r"call \.eval\(\) first$"),
    ("back S>stats", 0, lambda m: tb(m, BEL_BAD, ST[:1], CELL, SHIFT, TAPS, 0.0), V, r"score_prev must be \[B,512,512\] or \[B,1,512,512\], got \(2, 512, 511\)"),
    ("back stats>cell", 0, lambda m: tb(m, BEL, ST[:1], CELL.long(), SHIFT, TAPS, 0.0), V, r"prev_stats must be a float32 tensor \[2, 4\]"),
    ("back cell>taps", 0, lambda m: tb(m, BEL, ST, CELL.long(), SHIFT, TAPS_BAD, 0.0), V, r"cell must be an int32 tensor \[2\]"),
    ("back taps>floor", 0, lambda m: tb(m, BEL, ST, CELL, SHIFT, TAPS_BAD, -1.0), V, r"taps must be \[radius\+1\] or \[2, radius\+1\], got \(3, 4\)"),
    ("back floor>shift", 0, lambda m: tb(m, BEL, ST, CELL, SHIFT_BAD, TAPS, -1.0), V, r"floor must be >= 0"),
    ("back shift>D", 0, lambda m: tb(m, BEL, ST, CELL, SHIFT_BAD, TAPS, 0.0), V, r"shift_px must have shape \(2, 2\), got \(3, 2\)"),
    ("back ends", 0, lambda m: tb(m, BEL, ST, CELL, SHIFT, TAPS, 0.0), V, r"score_prev must be a cuda tensor, not a cpu tensor"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_error_precedence(case):
    _, training, call, exc, message = case
    with pytest.raises(exc, match=message):
        call(model(bool(training)))


# ---- the definition against a dense Viterbi ------------------------------------------------------------------------------------------

HMM_HW, HMM_T = 12, 5
HMM_SHIFTS = np.float32([[1.3, -2.4], [2.0, -1.0], [-2.7, 0.6], [0.25, 2.9]])       # one integer shift; all inside (-3, 3)
HMM_TAPS = aerial.gaussian_taps(0.9, 2)
HMM_FLOOR = np.float32(1e-3)


def test_definition_is_the_dense_viterbi_of_the_augmented_model():
    """5 frames on a 12 x 12 grid: the float64 definition, run on the dense filter's beliefs, walks the path of the textbook recursion
    over all 144 states with transition max(u, floor) - cells and link kinds."""
    n = HMM_HW * HMM_HW
    for seed in (5, 6, 7):
        like = np.random.default_rng(seed).uniform(0.05, 1.0, size=(HMM_T, n)) ** 4
        alpha, _ = smooth_ref.dense_forward_backward(like, HMM_SHIFTS, HMM_TAPS, float(HMM_FLOOR), HMM_HW)
        want_cells, want_kinds = viterbi_ref.dense_viterbi(like, HMM_SHIFTS, HMM_TAPS, float(HMM_FLOOR), HMM_HW)
        shifts = [None] + list(HMM_SHIFTS)
        cells, links, stats, _ = viterbi_ref.sweep([a.reshape(HMM_HW, HMM_HW) for a in alpha], shifts, HMM_TAPS, HMM_FLOOR, HMM_HW)
        assert cells.tolist() == want_cells.tolist(), (seed, cells, want_cells)
        assert links.tolist() == want_kinds.tolist(), (seed, links, want_kinds)
        assert stats[0, 3] == 1 and not stats[1:, 3].any() and ((stats[:, 1] >= 1) & (stats[:, 1] < 2)).all()


# ---- streams ---------------------------------------------------------------------------------------------------------------------

def test_crafted_stream_path_stays_on_the_truth():
    """Frames 2 .. 11 of tests/track_ref's stream in float64.  The filter has no prior for frame 2, a SEQ_STRONG frame: its argmax is the
    distractor, 306 px off.  The path is within 1 px of the truth in every frame and every link is a MOVE; from the second frame on the
    best score on the distractor is at most 3.6e-3 of the peak, so a float32 rounding cannot flip a cell."""
    frames, beliefs, cells, links, scores = viterbi_ref.crafted_path()
    first = frames[0]
    assert track_ref.pixel_distance(int(np.argmax(beliefs[0])), track_ref.sequence_truth(first)) > 300.0
    for t, k in enumerate(frames):
        assert track_ref.pixel_distance(int(cells[t]), track_ref.sequence_truth(k)) <= 1.0, (k, cells[t])
    assert links.tolist() == [viterbi_ref.START] + [viterbi_ref.MOVE] * (len(frames) - 1)
    dx, dy = (int(v) for v in track_ref.SEQ_DISTRACTOR)
    for t in range(1, len(frames)):
        assert scores[t][dy - 8:dy + 9, dx - 8:dx + 9].max() <= 3.6e-3 * scores[t].max(), t


def test_relocalisation_stream_jumps_once():
    truth, beliefs, cells, links, _ = viterbi_ref.reloc_path()
    for t in range(viterbi_ref.RELOC_T):
        assert track_ref.pixel_distance(int(cells[t]), truth[t]) <= 1.0, (t, cells[t], truth[t])
    want = [viterbi_ref.START] + [viterbi_ref.MOVE] * (viterbi_ref.RELOC_T - 1)
    want[5] = viterbi_ref.JUMP
    assert links.tolist() == want


def test_zero_belief_mid_stream_ends_one_segment_and_starts_the_next():
    """A frame without a finite posterior stores a zero belief, and the tracker feeds the frame after it through a flat prior: that
    frame's belief is its likelihood alone.  The zero frame has cell -1 and START on both sides, and each segment's cells are those of
    the segment run alone."""
    hw, T, z = 64, 7, 3
    taps, floor, step = aerial.gaussian_taps(1.0, 3), np.float32(1e-6), np.float32([3.3, 1.6])
    logits = [viterbi_ref.peak_logits((10 + 3.3 * k, 20 + 1.6 * k), hw) for k in range(T)]
    beliefs = viterbi_ref.filter_beliefs(logits[:z], step, taps, floor, hw) + [np.zeros((hw, hw))] + \
        viterbi_ref.filter_beliefs(logits[z + 1:], step, taps, floor, hw)
    shifts = [None] + [step] * (T - 1)
    cells, links, stats, _ = viterbi_ref.sweep(beliefs, shifts, taps, floor, hw)
    assert cells[z] == -1 and links[z] == viterbi_ref.START and links[z + 1] == viterbi_ref.START
    assert stats[z, 0] == -1 and np.isnan(stats[z, 1]) and stats[z, 3] == 0 and stats[z + 1, 3] == 1
    head, head_links, _, _ = viterbi_ref.sweep(beliefs[:z], shifts[:z], taps, floor, hw)
    tail, tail_links, _, _ = viterbi_ref.sweep(beliefs[z + 1:], [None] + shifts[z + 2:], taps, floor, hw)
    assert cells[:z].tolist() == head.tolist() and cells[z + 1:].tolist() == tail.tolist()
    assert links[:z].tolist() == head_links.tolist() and links[z + 1:].tolist() == tail_links.tolist()
    for t in list(range(z)) + list(range(z + 1, T)):
        assert track_ref.pixel_distance(int(cells[t]), (10 + 3.3 * t, 20 + 1.6 * t), hw) <= 1.0, t


# ---- map_path against a fake model ------------------------------------------------------------------------------------------------

def test_map_path_makes_the_calls_in_order(monkeypatch):
    T, B = 4, 2
    log = [(torch.full((B, 512, 512), float(t + 1)), None if t == 0 else np.full((B, 2), float(t)), np.ones(3, np.float32) * t, 1e-7 * t)
           for t in range(T)]
    calls = []

    def fake_step(model, belief, belief_prev=None, score_prev=None, prev_stats=None, shift_px=None, taps=None, floor=None, out=None):
        t = int(belief[0, 0, 0]) - 1
        calls.append(("step", t, None if belief_prev is None else int(belief_prev[0, 0, 0]) - 1,
                      None if score_prev is None else float(score_prev[0, 0, 0]), None if prev_stats is None else float(prev_stats[0, 2]),
                      None if shift_px is None else float(np.asarray(shift_px)[0, 0]), None if taps is None else float(taps[0]), floor))
        st = torch.tensor([[100.0 + t, 1.5, float(t), 0.0]] * B)
        return torch.full((B, 512, 512), 10.0 + t), st

    def fake_back(model, score_prev, prev_stats, cell, shift_px, taps, floor):
        assert cell.dtype == torch.int32 and tuple(cell.shape) == (B,)
        calls.append(("back", float(score_prev[0, 0, 0]), float(prev_stats[0, 2]), cell.tolist(), float(np.asarray(shift_px)[0, 0]), float(taps[0]), floor))
        return torch.tensor([[int(cell[0]) - 50, viterbi.LINK_MOVE], [int(cell[1]) - 60, viterbi.LINK_JUMP]], dtype=torch.int32)

    monkeypatch.setattr(viterbi, "track_viterbi", fake_step)
    monkeypatch.setattr(viterbi, "track_viterbi_back", fake_back)
    cells, links, stats, scores = viterbi.map_path(object(), log)
    assert calls[:T] == [("step", 0, None, None, None, None, None, None)] + \
        [("step", t, t - 1, 10.0 + t - 1, float(t - 1), float(t), float(t), 1e-7 * t) for t in range(1, T)]
    # T - 1 back calls, last link first: the last frame's cell is its own argmax (stats' index), every call takes the frame before's
    # score map and stats and the link's own predict arguments
    assert calls[T:] == [("back", 10.0 + t - 1, float(t - 1), [103 - 50 * (T - 1 - t), 103 - 60 * (T - 1 - t)], float(t), float(t), 1e-7 * t)
                         for t in range(T - 1, 0, -1)]
    assert cells.dtype == torch.int32 and links.dtype == torch.int32
    assert cells.tolist() == [[103 - 50 * (T - 1 - t), 103 - 60 * (T - 1 - t)] for t in range(T)]
    assert links.tolist() == [[viterbi.LINK_START] * B] + [[viterbi.LINK_MOVE, viterbi.LINK_JUMP]] * (T - 1)
    assert tuple(stats.shape) == (T, B, 4) and len(scores) == T and [float(s[0, 0, 0]) for s in scores] == [10.0, 11.0, 12.0, 13.0]
    with pytest.raises(ValueError, match="empty"):
        viterbi.map_path(object(), [])
    with pytest.raises(ValueError, match="no shift"):
        viterbi.map_path(object(), [log[0], log[0]])
