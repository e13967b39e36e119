"""The joint predict under an affine map per source heading bin on the device (ccvpe_track_joint_predict_affine): it
gives ccvpe_track_joint_predict's bits on integer translations, moves a quarter turn and a bin turn exactly, follows the float64
restatement tests/joint_affine_ref.py fed the float32 inputs the device got, shares its c with ccvpe_track_predict_affine, is two
launches with the same bits every time, isolates a degenerate query, refuses bad arguments with nothing launched, and with the
update separates the two peaks of the crafted turning stream as aerial.AffineJointTracker.

The bound against the restatement.  All terms are non-negative, so it is relative, u = 2^-24:
    A = the sampling and the xy pass             ccvpe_track_predict_affine's count (tests/test_track_affine_gpu.py)    4r + 12
    M[d], the chain, the floor                   ccvpe_track_joint_predict's count (tests/test_track_joint_gpu.py)      2rh + 6
so prior is within (4 r + 2 rh + 18) u of the restatement; the tests allow twice that, plus the coordinate term of the affine
predict, 2^-38 max(joint of the query): the float64 coordinates of the device (fused) and of the restatement differ by <= 2^-42 px.
Below 2^-100 the tests ask for a small value that is not NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial
from tests import joint_affine_ref as jar
from tests import joint_ref as jr
from tests import track_ref
from tests.test_track_joint_gpu import base, eq, predict_inputs

pytestmark = pytest.mark.gpu

N = 512 * 512
EPS = 2.0 ** -24
TINY = 2.0 ** -100
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
R = aerial.rigid_matrix
SHEAR = np.array([1.05, 0.31, -40.7, -0.12, 0.93, 22.15])
INT_SHIFTS = [(0, 0), (1, 0), (0, -1), (37, -120), (-255, 256), (511, 511), (-511, 3), (512, 0), (700, -900), (-3, 14), (8, 8)]


def translations(shift):
    s = np.asarray(shift, np.float64)
    m = np.zeros(s.shape[:-1] + (6,))
    m[..., 0] = m[..., 4] = 1.0
    m[..., 2], m[..., 5] = -s[..., 0], -s[..., 1]
    return m


# ---- 1. integer translations: the bits of track_joint_predict -------------------------------------------------------------------------

@pytest.mark.parametrize("nb,r,rh", [(4, 0, 0), (8, 6, 1), (6, 8, 2)])
def test_integer_translations_give_the_bits_of_track_joint_predict(nb, r, rh):
    m = base()["m"]
    j, _ = predict_inputs(nb)
    dev = torch.from_numpy(j).cuda()
    shift = np.array([[INT_SHIFTS[(4 * b + k) % len(INT_SHIFTS)] for k in range(nb)] for b in range(3)], np.float64)
    assert len({tuple(s) for s in shift[0]}) == nb                                    # a different shift per bin
    taps = aerial.gaussian_taps(1.0 + 0.3 * r, r)
    th = aerial.gaussian_taps(0.8, rh)
    w = 360.0 / nb
    for turn in (np.array([0.0, 2 * w, -w], np.float32), np.array([7.3, -33.0, 359.5], np.float32)):
        for floor in (0.0, 1e-9):
            got = m.track_joint_predict_affine(dev, translations(shift), taps, floor, turn, th)
            eq(got, m.track_joint_predict(dev, shift, taps, floor, turn, th))


# ---- 2. a quarter turn of the grid and a bin turn together, exact ----------------------------------------------------------------------

def test_quarter_turn_and_bin_turn_move_pixels_and_bins_exactly():
    """rigid_matrix(90, (0, 0)) turns the content a quarter turn counter-clockwise as displayed - torch.rot90(., 1), pinned in
    tests/test_track_joint_affine_cpu.py -, and with nb = 4 a turn of 90 degrees is one bin: prior[:, k] = rot90(joint[:, k - 1])."""
    m = base()["m"]
    j, _ = predict_inputs(4)
    dev = torch.from_numpy(j).cuda()
    mats = np.tile(R(90, (0, 0)), (4, 1))
    for floor in (0.0, 0.25, np.array([0.0, 1e-9, 1e-3], np.float32)):
        got = m.track_joint_predict_affine(dev, mats, [1.0], floor, 90.0, [1.0])
        fl = torch.as_tensor(np.broadcast_to(np.asarray(floor, np.float32), (3,)).copy()).cuda()[:, None, None]
        for k in range(4):
            eq(got[:, k], torch.rot90(dev[:, (k - 1) % 4], 1, (1, 2)) + fl)


# ---- 3. against the float64 restatement ------------------------------------------------------------------------------------------------

def check_against_ref(got, ref, joint, bound, what):
    """|got - ref| <= bound * ref + 2^-38 max(joint of the query) wherever ref >= 2^-100; below that got is small; no NaN.
    Returns worst error over bound."""
    got = np.asarray(got, np.float64).reshape(ref.shape)
    assert not np.isnan(got).any(), what
    absolute = np.broadcast_to(2.0 ** -38 * np.asarray(joint, np.float64).max(axis=(1, 2, 3))[:, None, None, None], ref.shape)
    big = ref >= TINY
    worst = float((np.abs(got - ref)[big] / (bound * ref[big] + absolute[big])).max()) if big.any() else 0.0
    print(f"{what}: {int(big.sum())} values checked, worst error / bound = {worst:.3f}")
    assert worst <= 1.0, (what, worst)
    assert (np.abs(got[~big]) <= 2.0 ** -99 + absolute[~big]).all(), what
    return worst


@pytest.mark.parametrize("case,nb,r,rh", [(0, 4, 0, 0), (1, 8, 1, 1), (2, 6, 8, 2), (3, 8, 8, 0)])
def test_predict_follows_the_float64_restatement(case, nb, r, rh):
    m = base()["m"]
    j, _ = predict_inputs(nb)
    dev = torch.from_numpy(j).cuda()
    # two queries with joint_matrix_table's matrices - a frame change and a body-frame motion -, rotations 0.5, 5, 37.5 and -171
    # degrees and the scales 0.8 and 1.25 over the four cases; one whose bins carry unrelated matrices
    rot = (0.5, 5.0, 37.5, -171.0)
    frames = np.stack([R(rot[case], [3.37, 0.81]), R(rot[(case + 1) % 4], [-4.25, 9.0], (0.8, 1.25)[case % 2])])
    shifts = aerial.joint_shift_table([6.0, -3.5], [0.5, 2.0], nb, zero_deg=(0.0, 90.0)[case % 2], clockwise=bool(case % 2))
    mats = np.empty((3, nb, 6))
    mats[:2] = aerial.joint_matrix_table(frames, shifts)
    loose = [SHEAR, np.zeros(6), R(37.5, [-30.6, 20.2], 1.25), translations([3.37, 0.81]), R(90.0, [0.5, -0.25]), R(-171.0, [7.77, 3.33], 0.8),
             np.array([-1.0, 0.0, 511.0, 0.0, 1.0, 0.0]), translations([600.0, 0.0])]
    mats[2] = np.stack(loose[:nb])
    turn = np.array([7.3, -400.25, 2 * 360.0 / nb], np.float32)
    floor = np.array([0.0, 1e-9, 1e-3], np.float32)
    taps = aerial.gaussian_taps(np.array([0.6, 1.5, 3.0]), r)
    th = aerial.gaussian_taps(np.array([0.5, 1.0, 2.0]), rh)
    got = m.track_joint_predict_affine(dev, mats, taps, floor, turn, th)
    assert got.shape == (3, nb, 512, 512) and got.dtype == torch.float32
    eq(m.track_joint_predict_affine(dev, torch.from_numpy(mats).cuda(), taps, floor, turn, th), got)      # the matrices on the device
    bound = 2 * (4 * r + 2 * rh + 18) * EPS
    check_against_ref(got.cpu().numpy(), jar.predict(j, mats, taps, turn, th, floor), j, bound, f"nb {nb} r {r} rh {rh}")


# ---- 4. one matrix for every bin: the c of the affine position predict -----------------------------------------------------------------

def test_one_matrix_for_every_bin_is_the_affine_position_predict_per_slice():
    """rh = 0, no turn, no floor: prior[:, k] is the c of track_predict_affine(joint[:, k]), so only the two logarithms differ -
    4 * 2^-24 |log| for logf, as much again for torch's"""
    m = base()["m"]
    nb = 4
    j, _ = predict_inputs(nb)
    dev = torch.from_numpy(j).cuda()
    M = R(5.0, [12.25, -7.5])
    taps = aerial.gaussian_taps(2.0, 6)
    prior = m.track_joint_predict_affine(dev, np.tile(M, (nb, 1)), taps, 0.0, 0.0, [1.0])
    worst = 0.0
    for k in range(nb):
        a = torch.log(prior[:, k]).double()
        b = m.track_predict_affine(dev[:, k].contiguous(), M, taps, 0.0).double()
        inf = torch.isinf(b)
        assert torch.equal(inf, torch.isinf(a)) and bool((a[inf] == b[inf]).all()) and not bool(torch.isnan(a).any())
        ratio = ((a - b).abs()[~inf] / (8 * EPS * b.abs()[~inf].clamp(min=1.0))).max().item()
        worst = max(worst, ratio)
    print(f"log(prior) against track_predict_affine: worst difference / bound = {worst:.3f}")
    assert worst <= 1.0


# ---- 5. forms and determinism ----------------------------------------------------------------------------------------------------------

def test_forms_share_their_bits_and_the_call_is_two_launches():
    m = base()["m"]
    nb, r, rh = 6, 3, 1
    j, _ = predict_inputs(nb)
    dev = torch.from_numpy(j).cuda()
    table = aerial.joint_matrix_table(R(5.0, [1.5, -2.0]), aerial.joint_shift_table(6.0, 0.5, nb))[0]
    taps, th = aerial.gaussian_taps(1.5, r), aerial.gaussian_taps(0.8, rh)
    turn, floor = np.array([7.3, -33.0, 120.0], np.float32), 1e-9
    got = m.track_joint_predict_affine(dev, table, taps, floor, turn, th)
    out = torch.empty_like(dev)
    res = m.track_joint_predict_affine(dev, table, taps, floor, turn, th, out=out)
    assert res is out
    eq(out, got)
    eq(m.track_joint_predict_affine(dev, np.broadcast_to(table, (3, nb, 6)), taps, floor, turn, th), got)
    eq(m.track_joint_predict_affine(dev, torch.from_numpy(table).cuda(), taps, floor, turn, th), got)
    eq(m.track_joint_predict_affine(dev, table, np.tile(taps, (3, 1)), np.full(3, floor, np.float32), torch.from_numpy(turn).cuda(), np.tile(th, (3, 1))), got)
    eq(m.track_joint_predict_affine(dev, table, taps, floor, turn, th), got)
    lib = _lib.load()
    torch.cuda.synchronize()
    n0 = lib.ccvpe_launch_count()
    m.track_joint_predict_affine(dev, table, taps, floor, turn, th)
    torch.cuda.synchronize()
    assert int(lib.ccvpe_launch_count() - n0) == 2


# ---- 6. degenerate queries ---------------------------------------------------------------------------------------------------------------

def test_degenerate_queries_give_the_floor_and_their_neighbour_keeps_its_bits():
    m = base()["m"]
    nb, r, rh = 4, 2, 1
    j, _ = predict_inputs(nb)
    j = np.stack([np.zeros_like(j[2]), j[2], j[2]])
    dev = torch.from_numpy(j).cuda()
    healthy = aerial.joint_matrix_table(R(37.5, [3.0, -2.0], 0.8), aerial.joint_shift_table(6.0, 0.5, nb))[0]
    mats = np.stack([healthy, np.zeros((nb, 6)), healthy])
    taps, th = aerial.gaussian_taps(1.0, r), aerial.gaussian_taps(0.8, rh)
    turn, floor = np.array([10.0, 20.0, 30.0], np.float32), np.array([1e-6, 0.25, 1e-9], np.float32)
    got = m.track_joint_predict_affine(dev, mats, taps, floor, turn, th)
    assert bool((got[0] == torch.tensor(1e-6, device="cuda")).all())                  # a zero joint: the floor everywhere
    assert bool((got[1] == 0.25).all())                                               # det = 0: the floor everywhere
    assert bool((got[2] > 1e-9).any()) and not bool(torch.isnan(got).any())
    alone = m.track_joint_predict_affine(dev[2:].contiguous(), mats[2:], taps, floor[2:], turn[2:], th)
    eq(got[2:], alone)


# ---- 7. the C ABI refuses, with nothing launched ----------------------------------------------------------------------------------------

def test_the_entry_point_refuses_bad_arguments_with_nothing_launched():
    m = base()["m"]
    lib = _lib.load()
    nb, B = 4, 1
    joint = torch.zeros(B, nb, 512, 512, device="cuda")
    prior = torch.zeros_like(joint)
    work = torch.empty(lib.ccvpe_track_joint_work_bytes(B, nb), dtype=torch.uint8, device="cuda")
    small = torch.zeros(64, device="cuda")
    mats = torch.from_numpy(np.tile(IDENTITY, (B, nb, 1))).cuda()
    h = m._handle
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def predict(joint=joint, batch=B, nb=nb, matrix=mats, taps=small, stride=0, radius=1, turn=small, htaps=small, hstride=0, rh=1, floor=small,
                work=work, prior=prior):
        return lib.ccvpe_track_joint_predict_affine(h, P(joint), batch, nb, P(matrix), P(taps), stride, radius, P(turn), P(htaps), hstride, rh,
                                                    P(floor), P(work), P(prior), None)

    torch.cuda.synchronize()
    n0 = lib.ccvpe_launch_count()
    for kw in ([dict(**{k: None}) for k in ("joint", "matrix", "taps", "turn", "htaps", "floor", "work", "prior")] +
               [dict(nb=3), dict(nb=73), dict(batch=0), dict(batch=8193), dict(radius=-1), dict(radius=33), dict(rh=-1), dict(rh=2), dict(rh=33, nb=72),
                dict(stride=1), dict(stride=3), dict(hstride=1), dict(hstride=3), dict(prior=joint), dict(prior=work), dict(work=joint)]):
        assert predict(**kw) == -1, kw
    torch.cuda.synchronize()
    assert int(lib.ccvpe_launch_count() - n0) == 0
    assert predict() == 0
    torch.cuda.synchronize()
    assert int(lib.ccvpe_launch_count() - n0) == 2
    assert not bool(prior.any())                                                      # a zero joint, zero taps and floors: zeros


# ---- 8. aerial.AffineJointTracker on the crafted turning stream --------------------------------------------------------------------------

class Held:
    """the model with a stream's crafted forward outputs in place of the network's"""

    def __init__(self, m, frames):
        self.m, self.frames, self.k = m, frames, 0

    def forward(self, grd, sat):
        lg, ori = self.frames[self.k]
        self.k += 1
        return lg, None, ori

    def __getattr__(self, name):
        return getattr(self.m, name)


def stream_frames():
    return [(torch.from_numpy(jar.sequence_logits(k)[None]).cuda(), torch.from_numpy(jar.sequence_ori(k).reshape(1, 2, 512, 512)).cuda())
            for k in range(jar.SEQ_FRAMES)]


def test_affine_joint_tracker_on_the_turning_two_peak_stream():
    """tests/joint_affine_ref's stream through aerial.AffineJointTracker: the bits of the spelled-out calls; each of the final shares
    of the marginal within 8 px of A and of B within T * (predict bound + update allowance) of the float64 stream's (0.999982 and
    6.1e-10, tests/test_track_joint_affine_cpu.py), relative to that share - T = 8 frames, the predict bound (4 r + 2 rh + 18) u, the
    marginal's allowance 2 (E + 4 u + (nb + 1) u) of tests/test_track_joint_gpu.py."""
    b0 = base()
    m, E, nb = b0["m"], b0["E"], jar.SEQ_BINS
    frame = jar.sequence_matrix()
    em = aerial.heading_emission(jar.SEQ_KAPPA, nb)
    taps = aerial.gaussian_taps(jar.SEQ_SIGMA, jar.SEQ_RADIUS)
    th = list(jar.SEQ_HTAPS)
    frames = stream_frames()
    grd, sat = torch.zeros(1, 3, 154, 231), torch.zeros(1, 3, 512, 512)
    # the float64 stream, and the spelled-out device calls
    table = aerial.joint_matrix_table(frame, aerial.joint_shift_table(jar.SEQ_FORWARD, 0.0, nb))
    turn = float(aerial.matrix_rotation_deg(frame))
    tr, held = aerial.AffineJointTracker(), Held(m, frames)
    ref_joint, joint = None, None
    for k in range(jar.SEQ_FRAMES):
        rows, marg, hist = tr.step(held, grd, em, frame, jar.SEQ_FORWARD, 0.0, 0.0, taps, th, jar.SEQ_FLOOR, sat=sat)
        lg, ori = frames[k]
        prior = None if joint is None else m.track_joint_predict_affine(joint, table, taps, jar.SEQ_FLOOR, turn, th)
        srows, joint, smarg, shist = m.track_joint_update_logits(lg, ori, em, prior)
        for a, b in ((rows, srows), (tr.joint, joint), (marg, smarg), (hist, shist)):
            eq(a, b)
        rp = None
        if ref_joint is not None:
            rp = jar.predict(ref_joint, table, taps, turn, jar.SEQ_HTAPS, jar.SEQ_FLOOR).astype(np.float32).reshape(1, nb, N)
        ref = jr.update(lg.cpu().numpy(), ori.cpu().numpy().reshape(1, 2, N), em, nb, rp)
        ref_joint = ref["joint"].astype(np.float32).reshape(1, nb, 512, 512)
    a, b = jar.sequence_peaks(jar.SEQ_FRAMES - 1)
    got = marg.cpu().numpy()
    near = [(jar.mass_near(got, p), jar.mass_near(ref["marginal"], p)) for p in (a, b)]
    T = jar.SEQ_FRAMES
    tol = T * ((4 * jar.SEQ_RADIUS + 2 * (len(th) - 1) + 18) * EPS + 2 * (E + 4 * EPS + (nb + 1) * EPS))
    for name, (dev_share, ref_share) in zip("AB", near):
        print(f"share of the marginal near {name}: device {dev_share:.9e}, float64 {ref_share:.9e}, "
              f"difference / (tolerance * share) = {abs(dev_share - ref_share) / (tol * ref_share):.3f}")
    assert near[0][1] > 0.99
    for dev_share, ref_share in near:
        assert abs(dev_share - ref_share) <= tol * ref_share
    assert track_ref.pixel_distance(int(rows[0, 0].item()), a) <= 1.0 and int(rows[0, 2].item()) == 1


def test_affine_joint_tracker_at_integer_translations_is_the_joint_tracker():
    """frames that differ by whole pixels and a vehicle that only turns: every bin's matrix is one integer translation, and the
    stream has the bits of aerial.JointTracker fed the same shifts through its window origins (25 map pixels = 16 output pixels)"""
    m = base()["m"]
    nb = jar.SEQ_BINS
    em = aerial.heading_emission(jar.SEQ_KAPPA, nb)
    taps = aerial.gaussian_taps(jar.SEQ_SIGMA, jar.SEQ_RADIUS)
    th = list(jar.SEQ_HTAPS)
    frames = stream_frames()[:3]
    grd, sat = torch.zeros(1, 3, 154, 231), torch.zeros(1, 3, 512, 512)
    origins = np.array([[800, 400], [825, 350], [775, 375]])
    ta, tj = aerial.AffineJointTracker(), aerial.JointTracker()
    ha, hj = Held(m, frames), Held(m, frames)
    for k in range(3):
        shift = np.zeros(2) if k == 0 else aerial.oxford_track_shift(origins[k - 1], origins[k], np.zeros(2))[0]
        assert (shift == np.round(shift)).all() and (k == 0 or shift.any())
        ra = ta.step(ha, grd, em, R(0.0, shift), 0.0, 0.0, 7.3, taps, th, jar.SEQ_FLOOR, sat=sat)
        rj = tj.step(hj, grd, em, 0.0, 0.0, 7.3, taps, th, jar.SEQ_FLOOR, sat=sat, origins=origins[k:k + 1])
        for a, b in zip(ra + (ta.joint,), rj + (tj.joint,)):
            eq(a, b)
