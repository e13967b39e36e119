"""The joint predict under an affine map per source heading bin without a GPU: the entry point is exported and
refuses bad arguments before it uses the handle; the model method checks its arguments without a device, in track_joint_predict's
order; the float64 restatement tests/joint_affine_ref.py is tests/joint_ref.predict on translations and turns a joint by a quarter
turn exactly; the host helpers (aerial.joint_matrix_table, aerial.matrix_rotation_deg) have their closed forms;
aerial.AffineJointTracker is forward + predict + update, against a stub model; and the restatement alone separates the two peaks of
the crafted turning stream where the position filter does not."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models
from tests import joint_affine_ref as jar
from tests import joint_ref as jr
from tests import track_affine_ref as ar
from tests import track_ref

EINVAL = -1
N = 512 * 512
NEW = ("ccvpe_track_joint_predict_affine",)


def _msg(lib):
    return (lib.ccvpe_last_error() or b"").decode()


# ---- C entry point -------------------------------------------------------------------------------------------------------------------

def test_entry_point_is_exported_and_bound(built_library):
    lib = C.CDLL(built_library)
    for n in NEW:
        assert hasattr(lib, n)
    assert set(NEW) <= {n for n, _, _ in _lib.SYMBOLS}
    sig = {n: a for n, _, a in _lib.SYMBOLS}
    assert len(sig["ccvpe_track_joint_predict_affine"]) == len(sig["ccvpe_track_joint_predict"]) == 16


def test_arguments_are_checked_before_the_handle(built_library):
    lib = _lib.load()
    keep = [(C.c_float * 32)() for _ in range(3)]
    p, q, w = (C.cast(a, C.c_void_p) for a in keep)

    def call(joint=p, batch=2, nb=8, matrix=p, taps=p, stride=0, radius=3, turn=p, htaps=p, hstride=0, rh=1, floor=p, work=w, prior=q):
        return lib.ccvpe_track_joint_predict_affine(None, joint, batch, nb, matrix, taps, stride, radius, turn, htaps, hstride, rh, floor,
                                                    work, prior, None)

    for kw, word in (("joint", "joint"), ("matrix", "matrix"), ("taps", "taps"), ("turn", "turn_deg"), ("htaps", "htaps"), ("floor", "floor"),
                     ("work", "work"), ("prior", "prior")):
        assert call(**{kw: None}) == EINVAL and word in _msg(lib) and "handle" not in _msg(lib), (kw, _msg(lib))
    # the order of ccvpe_track_joint_predict: the named pointers, nb, the batch, the radius, the stride, the heading radius and stride
    assert call(joint=None, matrix=None) == EINVAL and "joint" in _msg(lib)
    assert call(matrix=None, nb=3) == EINVAL and "matrix" in _msg(lib)
    assert call(nb=3, batch=0, radius=-1) == EINVAL and "nb" in _msg(lib)
    assert call(batch=0, radius=-1) == EINVAL and "batch" in _msg(lib)
    assert call(radius=-1, rh=9) == EINVAL and "radius" in _msg(lib) and "hradius" not in _msg(lib)
    assert call(rh=9, prior=p) == EINVAL and "hradius" in _msg(lib)
    for nb in (3, 0, -1, 73, 360):
        assert call(nb=nb, rh=0) == EINVAL and "nb" in _msg(lib), (nb, _msg(lib))
    for batch, nb in ((0, 8), (-1, 8), (4097, 8), (8193, 4), (456, 72)):
        assert call(batch=batch, nb=nb) == EINVAL and "batch" in _msg(lib), (batch, nb, _msg(lib))
    for r in (-1, 33):
        assert call(radius=r) == EINVAL and "radius" in _msg(lib), (r, _msg(lib))
    for s in (1, 3, 5, -4):
        assert call(stride=s) == EINVAL and "taps_stride" in _msg(lib), (s, _msg(lib))
    for nb, rh in ((8, -1), (8, 4), (4, 2), (72, 33), (6, 3)):
        assert call(nb=nb, rh=rh) == EINVAL and "hradius" in _msg(lib), (nb, rh, _msg(lib))
    for s in (1, 3, -2):
        assert call(hstride=s) == EINVAL and "htaps_stride" in _msg(lib), (s, _msg(lib))
    for kw in (dict(prior=p), dict(prior=w), dict(work=p)):
        assert call(**kw) == EINVAL and "alias" in _msg(lib), (kw, _msg(lib))
    assert call(joint=C.c_void_p(p.value + 4)) == EINVAL and "aligned" in _msg(lib)
    # valid arguments all the way: the null handle is the first thing refused
    for kw in (dict(), dict(nb=4, rh=1), dict(nb=6, rh=2), dict(nb=72, rh=32, hstride=33), dict(radius=0, stride=1), dict(radius=32, stride=33),
               dict(batch=4096, nb=8), dict(batch=455, nb=72, rh=0, hstride=1)):
        assert call(**kw) == EINVAL and "handle" in _msg(lib), (kw, _msg(lib))


# ---- the model method ----------------------------------------------------------------------------------------------------------------

def _model():
    return models.CVM_OxfordRobotCar("cpu").eval()


def test_method_refuses_bad_arguments_in_order():
    m = _model()
    nb = 6
    jt = torch.zeros(2, nb, 512, 512)
    ident = np.tile(np.array([1.0, 0, 0, 0, 1, 0]), (2, nb, 1))
    ok = dict(matrix=ident, taps=[1.0], floor=0.0, turn_deg=0.0, heading_taps=[1.0])

    def call(joint=jt, **kw):
        a = dict(ok)
        a.update(kw)
        return m.track_joint_predict_affine(joint, a["matrix"], a["taps"], a["floor"], a["turn_deg"], a["heading_taps"], out=a.get("out"))

    for bad in (torch.zeros(512, 512), torch.zeros(2, 512, 512), torch.zeros(2, nb, 512, 511), np.zeros((2, nb, 512, 512)),
                torch.zeros(2, 3, 512, 512), torch.zeros(1, 73, 1, 1).expand(1, 73, 512, 512)):
        with pytest.raises(ValueError, match="joint must"):
            call(bad)
    with pytest.raises(ValueError, match="joint must be float32"):
        call(jt.double())
    with pytest.raises(ValueError, match="joint must be contiguous"):
        call(jt.transpose(2, 3))
    for bad in (np.zeros(6), np.zeros((2, 6)), np.zeros((2, nb + 1, 6)), np.zeros((1, nb, 6)), np.zeros((2, nb, 5)), np.zeros((nb, 2, 6)), 1.0):
        with pytest.raises(ValueError, match=r"matrix must be \[6, 6\] or \[2, 6, 6\]"):
            call(matrix=bad)
    for v in (float("nan"), float("inf"), -float("inf")):
        bad = ident.copy()
        bad[1, 3, 2] = v
        for form in (bad, torch.from_numpy(bad), bad.tolist()):
            with pytest.raises(ValueError, match="matrix must be finite"):
                call(matrix=form)
    for bad in (np.zeros((3, 4)), np.zeros(0), np.zeros(34), 1.0):
        with pytest.raises(ValueError, match="taps"):
            call(taps=bad)
    for bad in (np.zeros((3, 2)), np.zeros(0), np.zeros(4), np.zeros(34), 1.0):              # 4 taps: 2 * 3 + 1 > 6 bins
        with pytest.raises(ValueError, match="heading_taps"):
            call(heading_taps=bad)
    for bad in (-1.0, float("nan"), np.zeros(3)):
        with pytest.raises(ValueError, match="floor"):
            call(floor=bad)
    with pytest.raises(ValueError, match="turn_deg"):
        call(turn_deg=np.zeros(3))
    for bad in (torch.zeros(2, nb + 1, 512, 512), torch.zeros(1, nb, 512, 512), torch.zeros(2, nb, 512, 512, dtype=torch.float64)):
        with pytest.raises(ValueError, match="out must"):
            call(out=bad)
    with pytest.raises(ValueError, match="out must not be the joint"):
        call(out=jt)
    # the order of track_joint_predict, the matrix where shift_px stands: joint, taps, floor, heading_taps, out, matrix, turn_deg
    nomat = np.zeros((2, nb, 5))
    with pytest.raises(ValueError, match="joint must"):
        call(torch.zeros(2, 512, 512), matrix=nomat, taps=1.0)
    with pytest.raises(ValueError, match="^taps must"):
        call(taps=1.0, matrix=nomat, floor=-1.0)
    with pytest.raises(ValueError, match="floor must"):
        call(floor=-1.0, matrix=nomat, heading_taps=np.zeros(4))
    with pytest.raises(ValueError, match="heading_taps"):
        call(heading_taps=np.zeros(4), matrix=nomat, out=jt)
    with pytest.raises(ValueError, match="out must"):
        call(out=jt, matrix=nomat)
    with pytest.raises(ValueError, match="matrix must be"):
        call(matrix=nomat, turn_deg=np.zeros(3), floor=np.zeros(3))
    with pytest.raises(ValueError, match="turn_deg"):
        call(turn_deg=np.zeros(3), floor=np.zeros(3))
    # accepted forms: the CPU joint is refused next
    for kw in (dict(), dict(matrix=ident[0]), dict(matrix=torch.from_numpy(ident)), dict(matrix=ident[0].tolist()),
               dict(taps=np.ones((2, 5), np.float32) / 9, heading_taps=torch.tensor([[0.5, 0.2, 0.05]] * 2), floor=np.full(2, 1e-6),
                    turn_deg=torch.tensor([3.0, -400.0])), dict(out=torch.zeros(2, nb, 512, 512), matrix=ident.astype(np.float32))):
        with pytest.raises(ValueError, match="joint must be a cuda tensor"):
            call(**kw)
    with pytest.raises(RuntimeError, match="eval"):
        _model().train().track_joint_predict_affine(jt, ident, [1.0], 0.0, 0.0, [1.0])
    # the method is the mixin's: _CVMBase's own method set stays as it was
    assert "track_joint_predict_affine" in vars(models._JointFilter) and "track_joint_predict_affine" not in vars(models._CVMBase)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------

def _translations(shift):
    s = np.asarray(shift, np.float64)
    m = np.zeros(s.shape[:-1] + (6,))
    m[..., 0] = m[..., 4] = 1.0
    m[..., 2], m[..., 5] = -s[..., 0], -s[..., 1]
    return m


def test_restatement_is_joint_ref_on_translations():
    nb = 4
    rng = np.random.default_rng(30)
    j = rng.uniform(0, 1, size=(1, nb, 512, 512)).astype(np.float32)
    j[0, 0] = 0
    j[0, 0, 50, 40] = 1.0
    taps, th = aerial.gaussian_taps(1.5, 2), np.array([0.6, 0.2], np.float32)
    integer = np.array([[[0, 0], [3, -2], [-17, 40], [511, -600]]], np.float32)
    # float32 shifts whose fraction of x - dx fits float32 (magnitude >= 1 or dyadic), as tests/test_track_affine_cpu.py takes them
    fractional = np.array([[[0.5, 0.0], [-2.25, 1.5], [3.37, 1.81], [-40.6, 70.2]]], np.float32)
    for shift, bound in ((integer, 0.0), (fractional, 1e-11)):
        for turn, floor in ((0.0, 0.0), (33.0, 1e-9), (-90.0, 0.25)):
            want = jr.predict(j, shift, taps, turn, th, floor)
            got = jar.predict(j, _translations(shift.astype(np.float64)), taps, turn, th, floor)
            err = float(np.abs(got - want).max() / want.max())
            print(f"shift {'integer' if bound == 0 else 'fractional'} turn {turn}: worst difference {err:.3e} of the maximum")
            assert err <= bound, (turn, err)


def test_quarter_turn_and_bin_turn_are_exact_in_the_restatement():
    """rigid_matrix(90, (0, 0)) turns the content by a quarter turn counter-clockwise as displayed (its docstring: as
    PIL.Image.rotate(90)): it is (0, -1, 511, 1, 0, 0), output (x, y) reads source (511 - y, x), which is np.rot90(m, 1) -
    rot90(m)[y, x] = m[x, 511 - y].  With nb = 4 a turn of 90 degrees is one bin: o = -1, f = 0, prior[k] = A[(k - 1) mod 4]."""
    m = aerial.rigid_matrix(90, (0, 0))
    np.testing.assert_array_equal(m, [0, -1, 511, 1, 0, 0])
    rng = np.random.default_rng(31)
    j = rng.uniform(0, 1, size=(2, 4, 512, 512)).astype(np.float32)
    floor = np.array([0.0, 0.25], np.float32)
    got = jar.predict(j, np.tile(m, (4, 1)), [1.0], 90.0, [1.0], floor)
    for k in range(4):
        want = np.rot90(j[:, (k - 1) % 4], 1, axes=(1, 2)).astype(np.float64) + floor.astype(np.float64)[:, None, None]
        np.testing.assert_array_equal(got[:, k], want)
    assert torch.equal(torch.rot90(torch.from_numpy(j[:, 2]), 1, (1, 2)), torch.from_numpy(np.rot90(j[:, 2], 1, axes=(1, 2)).copy()))


# ---- host helpers --------------------------------------------------------------------------------------------------------------------

def _apply(m, p):
    m, p = np.asarray(m, np.float64), np.asarray(p, np.float64)
    return np.stack([m[..., 0] * p[..., 0] + m[..., 1] * p[..., 1] + m[..., 2], m[..., 3] * p[..., 0] + m[..., 4] * p[..., 1] + m[..., 5]], axis=-1)


def test_matrix_rotation_deg_recovers_rigid_matrix_s_angle():
    for deg in (0.0, 0.5, 5.0, 37.5, 90.0, -90.0, -171.0, 179.0, 180.0):
        for scale in (1.0, 0.8, 1.25):
            got = aerial.matrix_rotation_deg(aerial.rigid_matrix(deg, (13.5, -7.25), scale))
            assert np.ndim(got) == 0 and abs(float(got) - deg) <= 1e-12, (deg, scale, got)
    batch = aerial.rigid_matrix(np.array([10.0, -20.0, 135.0]), np.zeros((3, 2)), np.array([1.0, 2.0, 0.5]))
    np.testing.assert_allclose(aerial.matrix_rotation_deg(batch), [10.0, -20.0, 135.0], atol=1e-12)
    # composing turns adds their angles, inverting negates them
    a, b = aerial.rigid_matrix(25.0, (3, 4)), aerial.rigid_matrix(-60.5, (-8, 1), 1.1)
    assert abs(aerial.matrix_rotation_deg(aerial.affine_compose(a, b)) - (-35.5)) <= 1e-12
    assert abs(aerial.matrix_rotation_deg(aerial.affine_invert(b)) - 60.5) <= 1e-12
    # a sheared map: the rotation of the polar part, L = Q S with S symmetric positive definite
    q = np.radians(30.0)
    Q = np.array([[np.cos(q), -np.sin(q)], [np.sin(q), np.cos(q)]])        # rigid_matrix(30)'s linear part
    L = Q @ np.array([[1.3, 0.4], [0.4, 0.9]])
    assert abs(aerial.matrix_rotation_deg([L[0, 0], L[0, 1], 5.0, L[1, 0], L[1, 1], -2.0]) - 30.0) <= 1e-12
    assert aerial.matrix_rotation_deg(np.zeros(6)) == 0.0
    for bad in (np.zeros(5), np.zeros((2, 2, 6)), [1, 0, 0, 0, 1, float("nan")]):
        with pytest.raises(ValueError, match="matrix"):
            aerial.matrix_rotation_deg(bad)


def test_joint_matrix_table_closed_form():
    nb = 8
    d = aerial.joint_shift_table([10.0, 4.0], [0.0, -1.5], nb)
    frame = aerial.rigid_matrix(np.array([12.0, -30.0]), np.array([[3.0, -2.0], [0.0, 7.5]]), np.array([1.0, 0.9]))
    t = aerial.joint_matrix_table(frame, d)
    assert t.shape == (2, nb, 6) and t.dtype == np.float64
    np.testing.assert_array_equal(t[:, :, [0, 1, 3, 4]], np.broadcast_to(frame[:, None, [0, 1, 3, 4]], (2, nb, 4)))
    np.testing.assert_array_equal(t[:, :, 2], frame[:, None, 2] - d[:, :, 0])
    np.testing.assert_array_equal(t[:, :, 5], frame[:, None, 5] - d[:, :, 1])
    # the source of an output pixel is M(p_out) - d[k]: the frame change first, then the translation by -d in the old grid
    for b in range(2):
        for k in range(nb):
            back = np.array([1.0, 0.0, -d[b, k, 0], 0.0, 1.0, -d[b, k, 1]])
            np.testing.assert_allclose(t[b, k], aerial.affine_compose(back, frame[b]), rtol=0, atol=1e-12)
    # content at p_old with heading k ends at the new pixel that shows p_old + d[k]: the inverse table maps it there
    p_old = np.array([200.0, 310.0])
    for k in (0, 3):
        p_new = _apply(aerial.affine_invert(frame[0]), p_old + d[0, k])
        np.testing.assert_allclose(_apply(t[0, k], p_new), p_old, atol=1e-9)
    # no frame change: track_joint_predict's shift table as matrices
    ident = np.array([1.0, 0, 0, 0, 1, 0])
    np.testing.assert_array_equal(aerial.joint_matrix_table(ident, d), _translations(d))
    # one matrix for every query, one table for every matrix, a single query's [nb, 2]
    assert aerial.joint_matrix_table(frame[0], d).shape == (2, nb, 6)
    assert aerial.joint_matrix_table(frame, d[:1]).shape == (2, nb, 6)
    assert aerial.joint_matrix_table(frame[0], d[0]).shape == (1, nb, 6)
    # clockwise labels (Oxford's: 0 = north = up): the table carries the convention, the matrices only subtract it
    dc = aerial.joint_shift_table(6.0, 0.0, nb, zero_deg=90.0, clockwise=True)
    tc = aerial.joint_matrix_table(aerial.rigid_matrix(90, (0, 0)), dc)
    np.testing.assert_array_equal(tc[0, :, 2], 511.0 - dc[0, :, 0])
    np.testing.assert_array_equal(tc[0, :, 5], 0.0 - dc[0, :, 1])
    assert dc[0, 0, 1] < -5.5                                            # label 22.5 is mostly north: up, -y
    for kw, word in ((dict(shift_table=np.zeros((nb, 3))), "shift_table"), (dict(shift_table=np.zeros(2)), "shift_table"),
                     (dict(shift_table=np.full((1, nb, 2), np.nan)), "finite"), (dict(matrix=np.zeros(5)), "matrix"),
                     (dict(matrix=np.zeros((3, 6)), shift_table=np.zeros((2, nb, 2))), "rows")):
        args = dict(matrix=ident, shift_table=d)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            aerial.joint_matrix_table(**args)


# ---- aerial.AffineJointTracker against a stub model ---------------------------------------------------------------------------------

class _Stub:
    """records the calls a tracker step makes and returns tensors of the right shapes"""

    def __init__(self, nb):
        self.nb, self.calls = nb, []

    def forward_cached(self, grd, cache, tile_index=None):
        self.calls.append(("forward_cached", tile_index))
        B = grd.shape[0]
        return (torch.zeros(B, N), torch.zeros(B, 1, 512, 512), torch.ones(B, 2, 512, 512))

    def forward(self, grd, sat):
        self.calls.append(("forward",))
        B = grd.shape[0]
        return (torch.zeros(B, N), torch.zeros(B, 1, 512, 512), torch.ones(B, 2, 512, 512))

    def track_joint_predict_affine(self, joint, matrix, taps, floor, turn_deg, heading_taps, out=None):
        self.calls.append(("predict", joint, np.array(matrix), taps, floor, turn_deg, heading_taps))
        return torch.full_like(joint, 2.0)

    def track_joint_update_logits(self, logits, ori, emission, prior=None, out=None):
        self.calls.append(("update", prior, out))
        B = logits.shape[0]
        joint = out if out is not None else torch.zeros(B, self.nb, 512, 512)
        return torch.zeros(B, 5), joint, torch.full((B, 512, 512), 1.0 / N), torch.zeros(B, self.nb)

    def belief_summary(self, belief, radius):
        self.calls.append(("summary", belief, radius))
        return torch.zeros(belief.shape[0], 16)

    def belief_credible(self, belief, levels):
        self.calls.append(("credible", belief, levels))
        return torch.zeros(belief.shape[0], 4 + 3 * len(levels))


def test_affine_joint_tracker_is_forward_predict_update():
    nb = 8
    st = _Stub(nb)
    tr = aerial.AffineJointTracker()
    em = aerial.heading_emission(2.0, nb)
    taps, ht = aerial.gaussian_taps(2.0, 6), [0.8, 0.1]
    g = torch.zeros(2, 3, 154, 231)
    sat = torch.zeros(2, 3, 512, 512)
    frame = aerial.rigid_matrix(np.array([12.0, -30.0]), np.array([[3.0, -2.0], [0.0, 7.5]]))
    res = tr.step(st, g, em, frame, 5.0, 0.5, 3.0, taps, ht, 1e-9, sat=sat)
    assert len(res) == 3 and res[0].shape == (2, 5) and res[1].shape == (2, 512, 512) and res[2].shape == (2, nb)
    assert [c[0] for c in st.calls] == ["forward", "update"] and st.calls[1][1] is None            # the first step has no prior
    assert tr.joint.shape == (2, nb, 512, 512)
    st.calls.clear()
    held = tr.joint
    res = tr.step(st, g, em, frame, 5.0, 0.5, 3.0, taps, ht, 1e-9, sat=sat, summary_radius=8, credible_levels=[0.5, 0.9])
    assert [c[0] for c in st.calls] == ["forward", "predict", "update", "summary", "credible"]
    pred = st.calls[1]
    assert pred[1] is held and pred[2].shape == (2, nb, 6) and pred[3] is taps and pred[4] == 1e-9 and pred[6] is ht
    np.testing.assert_array_equal(pred[2], aerial.joint_matrix_table(frame, aerial.joint_shift_table(5.0, 0.5, nb)))
    # counter-clockwise labels: the grid's rotation is added to the vehicle's turn
    np.testing.assert_allclose(pred[5], [3.0 + 12.0, 3.0 - 30.0], rtol=0, atol=1e-12)
    assert st.calls[2][1] is st.calls[2][2] and bool((st.calls[2][1] == 2.0).all())           # the update runs in place on the prior
    assert tr.joint is st.calls[2][1]
    assert len(res) == 5 and res[3].shape == (2, 16) and res[4].shape == (2, 10)
    assert st.calls[3][1] is res[1] and st.calls[4][1] is res[1]                                # ... of the marginal
    # clockwise labels (zero_deg 90): the table takes the convention, the rotation is subtracted; one matrix, a cache, per-query turns
    st.calls.clear()
    one = aerial.rigid_matrix(7.5, (0, 0), 1.25)
    tr.step(st, g, em, one, [5.0, 2.0], 0.0, np.array([1.0, -2.0]), taps, ht, 1e-9, cache=torch.zeros(4), tile_index=[0, 1], zero_deg=90.0,
            clockwise=True)
    assert [c[0] for c in st.calls] == ["forward_cached", "predict", "update"] and st.calls[0][1] == [0, 1]
    np.testing.assert_array_equal(st.calls[1][2], aerial.joint_matrix_table(one, aerial.joint_shift_table([5.0, 2.0], 0.0, nb, 90.0, True)))
    np.testing.assert_allclose(st.calls[1][5], [1.0 - 7.5, -2.0 - 7.5], rtol=0, atol=1e-12)
    # a number stays a number, a tensor stays a tensor
    st.calls.clear()
    tr.step(st, g, em, one, 5.0, 0.0, 0.0, taps, ht, 1e-9, sat=sat)
    assert isinstance(st.calls[1][5], float) and abs(st.calls[1][5] - 7.5) <= 1e-12
    st.calls.clear()
    tr.step(st, g, em, one, 5.0, 0.0, torch.tensor([1.0, 2.0]), taps, ht, 1e-9, sat=sat)
    assert isinstance(st.calls[1][5], torch.Tensor) and torch.allclose(st.calls[1][5], torch.tensor([8.5, 9.5]))
    with pytest.raises(ValueError, match="streams"):
        tr.step(st, torch.zeros(3, 3, 154, 231), em, one, 5.0, 0.5, 3.0, taps, ht, 1e-9, sat=torch.zeros(3, 3, 512, 512))
    with pytest.raises(ValueError, match="bins"):
        tr.step(st, g, aerial.heading_emission(2.0, 6), one, 5.0, 0.5, 3.0, taps, ht, 1e-9, sat=sat)
    with pytest.raises(ValueError, match="one of the two"):
        tr.step(st, g, em, one, 5.0, 0.5, 3.0, taps, ht, 1e-9)
    with pytest.raises(ValueError, match="tile_index"):
        tr.step(st, g, em, one, 5.0, 0.5, 3.0, taps, ht, 1e-9, sat=sat, tile_index=[0, 1])
    tr.reset()
    assert tr.joint is None
    st.calls.clear()
    tr.step(st, g, em, None, 5.0, 0.5, 3.0, taps, ht, 1e-9, sat=sat)                              # the first step ignores the motion
    assert [c[0] for c in st.calls] == ["forward", "update"]


# ---- the crafted turning stream: the restatement alone ---------------------------------------------------------------------------------

def test_the_restatement_separates_the_two_peaks_across_turning_frames_and_the_position_filter_does_not():
    """tests/joint_ref's two peaks on frames that turn by 4 degrees each: A moves by the step in the world, B by minus the step, the
    field says the step's heading as each frame's grid labels it.  The float64 joint filter ends with 0.999982 of the marginal
    within 8 px of A and 6.1e-10 near B, the best bin having moved from 0 to 1 with the grid; the float64 position filter fed the
    frame change alone keeps 0.5056 near A and 0.4942 near B."""
    nb = jar.SEQ_BINS
    frame = jar.sequence_matrix()
    np.testing.assert_allclose(frame, aerial.rigid_matrix(jar.SEQ_TURN_DEG, (0.0, 0.0)), rtol=0, atol=1e-12)
    shifts = aerial.joint_shift_table(jar.SEQ_FORWARD, 0.0, nb)
    np.testing.assert_allclose(shifts[0, 0], jar.sequence_step(), rtol=0, atol=1e-12)
    table = aerial.joint_matrix_table(frame, shifts)
    turn = float(aerial.matrix_rotation_deg(frame))
    assert abs(turn - jar.SEQ_TURN_DEG) <= 1e-12
    em = aerial.heading_emission(jar.SEQ_KAPPA, nb)
    taps = aerial.gaussian_taps(jar.SEQ_SIGMA, jar.SEQ_RADIUS)
    joint, bel = None, None
    for k in range(jar.SEQ_FRAMES):
        lg, ori = jar.sequence_logits(k)[None], jar.sequence_ori(k)[None]
        prior = None
        if joint is not None:
            prior = jar.predict(joint, table, taps, turn, jar.SEQ_HTAPS, jar.SEQ_FLOOR).astype(np.float32).reshape(1, nb, N)
        r = jr.update(lg, ori, em, nb, prior)
        joint = r["joint"].astype(np.float32).reshape(1, nb, 512, 512)
        lp = None if bel is None else ar.predict(bel, frame, taps, jar.SEQ_FLOOR).astype(np.float32).reshape(1, N)
        bel = track_ref.update(lg, ori, lp)[2].astype(np.float32).reshape(1, 512, 512)
    a, b = jar.sequence_peaks(jar.SEQ_FRAMES - 1)
    near_a, near_b = jar.mass_near(r["marginal"], a), jar.mass_near(r["marginal"], b)
    pa, pb = jar.mass_near(bel, a), jar.mass_near(bel, b)
    print(f"joint filter: {near_a:.6f} near A, {near_b:.2e} near B; position filter: {pa:.4f} near A, {pb:.4f} near B")
    assert near_a > 0.99
    assert 0.4 < pa < 0.6 and 0.4 < pb < 0.6
    assert track_ref.pixel_distance(int(r["rows"][0, 0]), a) <= 1.0 and int(r["rows"][0, 2]) == 1
