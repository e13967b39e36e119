"""The affine predict step without a GPU (ccvpe_track_predict_affine): the C entry point and its argument checks (all
made before the handle is used), the model method's refusals, the numpy restatement tests/track_affine_ref.py against
tests/track_ref.py on translations, the affine helpers of ccvpe_amd.aerial against closed forms, the KITTI track matrix against the
Pillow restatement tests/pil_warp.py on synthetic tiles, and the crafted turning stream of the GPU filter test."""
import ctypes as C

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, aerial, models
from tests import pil_warp, track_affine_ref, track_ref

EINVAL = -1
N = 512 * 512
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])


# ---- C entry point -------------------------------------------------------------------------------------------------------------

def test_affine_entry_point_is_exported_and_bound(built_library):
    lib = C.CDLL(built_library)
    assert hasattr(lib, "ccvpe_track_predict_affine")
    assert "ccvpe_track_predict_affine" in {n for n, _, _ in _lib.SYMBOLS}


def _msg(lib):
    return (lib.ccvpe_last_error() or b"").decode()


def test_affine_predict_arguments_are_checked_before_the_handle(built_library):
    lib = _lib.load()
    a, b = (C.c_float * 16)(), (C.c_float * 16)()
    p, q = C.cast(a, C.c_void_p), C.cast(b, C.c_void_p)
    m = C.cast((C.c_double * 12)(), C.c_void_p)

    def call(belief=p, batch=2, matrix=m, taps=p, stride=0, radius=3, floor=p, out=q):
        return lib.ccvpe_track_predict_affine(None, belief, batch, matrix, taps, stride, radius, floor, out, None)

    for kw, word in (("belief", "belief"), ("matrix", "matrix"), ("taps", "taps"), ("floor", "floor"), ("out", "log_prior")):
        assert call(**{kw: None}) == EINVAL and word in _msg(lib), (kw, _msg(lib))
    for r in (-1, 33, 1000):
        assert call(radius=r) == EINVAL and "radius" in _msg(lib), (r, _msg(lib))
    for s in (1, 3, 5, -4):
        assert call(stride=s) == EINVAL and "taps_stride" in _msg(lib), (s, _msg(lib))
    for batch in (0, -1, 4097):
        assert call(batch=batch) == EINVAL and "batch" in _msg(lib), (batch, _msg(lib))
    assert call(out=p) == EINVAL and "alias" in _msg(lib)
    for r, s in ((0, 0), (0, 1), (3, 4), (32, 0), (32, 33)):
        assert call(radius=r, stride=s) == EINVAL and "handle" in _msg(lib), (r, s, _msg(lib))
    assert call(batch=4096) == EINVAL and "handle" in _msg(lib)


# ---- model method --------------------------------------------------------------------------------------------------------------

def _model():
    return models.CVM_KITTI("cpu").eval()


def test_affine_predict_method_refuses_bad_arguments():
    m = _model()
    bel = torch.zeros(3, 512, 512)
    mat = np.tile(IDENTITY, (3, 1))
    for bad in (torch.zeros(512, 512), torch.zeros(3, 512, 511), torch.zeros(3, 2, 512, 512), torch.zeros(3, N), np.zeros((3, 512, 512))):
        with pytest.raises(ValueError, match="belief must be"):
            m.track_predict_affine(bad, mat, [1.0], 0.0)
    with pytest.raises(ValueError, match="belief must be float32"):
        m.track_predict_affine(bel.double(), mat, [1.0], 0.0)
    with pytest.raises(ValueError, match="belief must be contiguous"):
        m.track_predict_affine(bel.transpose(1, 2), mat, [1.0], 0.0)
    for bad in (np.zeros((2, 6)), np.zeros((3, 5)), np.zeros(5), np.zeros((3, 2, 3)), np.zeros((1, 6)), 1.0):
        with pytest.raises(ValueError, match="matrix must be"):
            m.track_predict_affine(bel, bad, [1.0], 0.0)
    for v in (np.nan, np.inf, -np.inf):
        for k in (0, 2, 5):
            bad = mat.copy()
            bad[1, k] = v
            with pytest.raises(ValueError, match="matrix must be finite"):
                m.track_predict_affine(bel, bad, [1.0], 0.0)
            with pytest.raises(ValueError, match="matrix must be finite"):
                m.track_predict_affine(bel, torch.from_numpy(bad[1]), [1.0], 0.0)
    for bad in (np.zeros((2, 4)), np.zeros((3, 2, 2)), np.zeros(0), np.zeros(34), 1.0):
        with pytest.raises(ValueError, match="taps"):
            m.track_predict_affine(bel, mat, bad, 0.0)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="floor"):
            m.track_predict_affine(bel, mat, [1.0], bad)
    with pytest.raises(ValueError, match="floor"):
        m.track_predict_affine(bel, mat, [1.0], np.zeros(2))
    # accepted shapes: the CPU belief is refused next
    for matrix in (mat, IDENTITY, IDENTITY.tolist(), torch.from_numpy(mat), mat.astype(np.float32)):
        for taps in ([1.0], np.ones((3, 5), np.float32) / 9, torch.ones(33) / 65):
            for floor in (0.0, 1e-9, np.full(3, 1e-6), torch.zeros(3)):
                with pytest.raises(ValueError, match="belief must be a cuda tensor"):
                    m.track_predict_affine(bel, matrix, taps, floor)
    with pytest.raises(ValueError, match="belief must be a cuda tensor"):
        m.track_predict_affine(bel.view(3, 1, 512, 512), mat, [1.0], 0.0)
    with pytest.raises(RuntimeError, match="eval"):
        _model().train().track_predict_affine(bel, mat, [1.0], 0.0)


def test_affine_tracker_checks_its_arguments():
    t = aerial.AffineTracker()
    assert t.belief is None
    g, s = torch.zeros(2, 3, 256, 1024), torch.zeros(2, 3, 512, 512)
    with pytest.raises(ValueError, match="sat or as cache"):
        t.step(_model(), g, None, IDENTITY, [1.0], 0.0)
    with pytest.raises(ValueError, match="sat or as cache"):
        t.step(_model(), g, s, IDENTITY, [1.0], 0.0, cache=torch.zeros(16))
    with pytest.raises(ValueError, match="tile_index"):
        t.step(_model(), g, s, IDENTITY, [1.0], 0.0, tile_index=[0, 1])
    t.belief = torch.zeros(3, 512, 512)
    with pytest.raises(ValueError, match="streams"):
        t.step(_model(), g, s, IDENTITY, [1.0], 0.0)
    t.reset()
    assert t.belief is None


# ---- the restatement against tests/track_ref on translations -------------------------------------------------------------------

def _translation(shift):
    sh = np.asarray(shift, np.float32).astype(np.float64).reshape(-1, 2)
    out = np.tile(IDENTITY, (sh.shape[0], 1))
    out[:, 2], out[:, 5] = -sh[:, 0], -sh[:, 1]
    return out


@pytest.mark.parametrize("radius", [0, 3])
def test_restatement_is_track_ref_on_translations(radius):
    hw = 96
    rng = np.random.default_rng(21)
    taps = aerial.gaussian_taps(1.5, radius)
    integer = [[0, 0], [3, -2], [-17, 40], [95, 0], [0, -96], [200, 5]]
    # float32 shifts of magnitude >= 1, or dyadic ones: the fraction of x - dx then fits float32, so that the restatement's rounding of
    # the fraction (which tests/track_ref does not have) changes nothing and only the order of the sums differs
    fractional = [[0.5, 0.0], [-2.25, 1.5], [3.37, 1.81], [-40.6, 70.2], [95.5, -0.125], [1.001, -1.999]]
    for shifts, bound in ((integer, 0.0), (fractional, 1e-11)):
        bel = rng.uniform(0, 1, size=(len(shifts), hw, hw)).astype(np.float32)
        bel[0] = 0
        bel[0, 50, 40] = 1.0
        want = track_ref.predict_c(bel, shifts, taps, hw)
        got = track_affine_ref.predict_c(bel, _translation(shifts), taps, hw)
        err = np.abs(got - want).max() / bel.max()
        print(f"radius {radius}: max |affine restatement - track_ref| / max = {err:.3g}")
        assert err <= bound, (radius, err)


def test_restatement_on_crafted_maps():
    hw = 96
    d = np.zeros((1, hw, hw), np.float32)
    d[0, 50, 40] = 1.0
    # M maps an output index to the source position: output (47, 47) reads (40, 50)
    c = track_affine_ref.predict_c(d, [1, 0, -7, 0, 1, 3], [1.0], hw)
    assert c[0, 47, 47] == 1.0 and c.sum() == 1.0
    # a quarter turn about the centre: integer positions, pixels move exactly
    rng = np.random.default_rng(2)
    b = rng.uniform(0, 1, size=(1, hw, hw)).astype(np.float32)
    m = aerial.rigid_matrix(90, [0, 0], centre=((hw - 1) / 2, (hw - 1) / 2))
    np.testing.assert_array_equal(track_affine_ref.predict_c(b, m, [1.0], hw)[0], np.rot90(b[0], 1).astype(np.float64))
    # |det| keeps the mass of a blob inside the window: content shrunk to 0.8 and grown to 1.25, turned by 30 degrees
    y, x = np.mgrid[0:hw, 0:hw]
    blob = np.exp(-((x - 50.0) ** 2 + (y - 44.0) ** 2) / 50.0).astype(np.float32)[None]
    for scale in (0.8, 1.25):
        m = aerial.rigid_matrix(30, [2.5, -1.25], scale, centre=(47.5, 47.5))
        c = track_affine_ref.predict_c(blob, m, [1.0], hw)
        assert c.sum() == pytest.approx(blob.sum(dtype=np.float64), rel=2e-3)
    # a degenerate matrix, and positions far outside (clipped after the neighbour offset: nothing leaks in from column 0)
    b[0, :, 0] = 1.0
    assert track_affine_ref.predict_c(b, np.zeros(6), [0.5, 0.25], hw).sum() == 0.0
    for far in ([1, 0, -1e6, 0, 1, 0], [1, 0, -7.5, 0, 1, 0], [1, 0, 0, 0, 1, 1e300]):
        c = track_affine_ref.predict_c(b, far, [1.0], hw)
        assert (c[0, :, :6] == 0).all(), far
    assert np.isneginf(track_affine_ref.predict(b, np.zeros(6), [1.0], 0.0, hw)).all()
    assert (track_affine_ref.predict(b, np.zeros(6), [1.0], 0.25, hw) == np.log(0.25)).all()


# ---- helpers -------------------------------------------------------------------------------------------------------------------

def _apply(m, pts):
    m = np.asarray(m, np.float64)
    pts = np.asarray(pts, np.float64)
    return np.stack([m[..., 0] * pts[..., 0] + m[..., 1] * pts[..., 1] + m[..., 2],
                     m[..., 3] * pts[..., 0] + m[..., 4] * pts[..., 1] + m[..., 5]], axis=-1)


def test_compose_and_invert():
    rng = np.random.default_rng(8)
    m = rng.uniform(-2, 2, size=(20, 6))
    m[:, [0, 4]] += 3.0          # well away from singular
    np.testing.assert_allclose(aerial.affine_compose(aerial.affine_invert(m), m), np.tile(IDENTITY, (20, 1)), atol=1e-12)
    np.testing.assert_allclose(aerial.affine_compose(m, aerial.affine_invert(m)), np.tile(IDENTITY, (20, 1)), atol=1e-12)
    assert aerial.affine_compose(aerial.affine_invert(m[0]), m[0]).shape == (6,)
    # compose(a, b) applies b first
    a, b = m[:10], m[10:]
    pts = rng.uniform(-100, 600, size=(10, 2))
    np.testing.assert_allclose(_apply(aerial.affine_compose(a, b), pts), _apply(a, _apply(b, pts)), rtol=1e-12, atol=1e-9)
    # one matrix against a batch
    np.testing.assert_allclose(aerial.affine_compose(a[0], b), aerial.affine_compose(np.tile(a[0], (10, 1)), b), rtol=0, atol=0)
    with pytest.raises(ValueError, match="singular"):
        aerial.affine_invert([1, 2, 0, 2, 4, 0])
    with pytest.raises(ValueError, match="finite"):
        aerial.affine_invert([1, 0, np.nan, 0, 1, 0])
    with pytest.raises(ValueError, match="must be"):
        aerial.affine_compose(np.zeros(5), IDENTITY)


def test_index_form_round_trips_and_matches_the_pixel_centre_convention():
    rng = np.random.default_rng(9)
    m = rng.uniform(-2, 2, size=(7, 6))
    np.testing.assert_allclose(aerial.affine_pillow_form(aerial.affine_index_form(m)), m, rtol=0, atol=1e-15)
    np.testing.assert_allclose(aerial.affine_index_form(aerial.affine_pillow_form(m)), m, rtol=0, atol=1e-15)
    # Pillow: centre (x + .5, y + .5) -> position q whose pixel centres are at i + .5; index form: x -> q - .5
    pts = rng.uniform(0, 500, size=(7, 2))
    np.testing.assert_allclose(_apply(aerial.affine_index_form(m), pts), _apply(m, pts + 0.5) - 0.5, rtol=1e-13, atol=1e-10)
    # a translation is the same in both; Pillow's rotation about (W/2, H/2) is a rotation about index (W/2 - .5, H/2 - .5)
    np.testing.assert_array_equal(aerial.affine_index_form([1, 0, 7, 0, 1, -3]), [1, 0, 7, 0, 1, -3])
    rot = aerial.affine_index_form(aerial.rotate_matrix(33.0, 512, 512))
    np.testing.assert_allclose(_apply(rot, [255.5, 255.5]), [255.5, 255.5], atol=1e-12)
    np.testing.assert_allclose(rot, aerial.rigid_matrix(33.0, [0, 0]), atol=1e-12)     # PIL.Image.rotate's sense of rotation


def test_rigid_matrix_closed_forms():
    np.testing.assert_array_equal(aerial.rigid_matrix(0, [3.25, -7.5]), [1, 0, -3.25, 0, 1, 7.5])
    out = aerial.rigid_matrix(0, [[1, 2], [3, 4]])
    np.testing.assert_array_equal(out, [[1, 0, -1, 0, 1, -2], [1, 0, -3, 0, 1, -4]])
    corners = np.array([[0, 0], [511, 0], [511, 511], [0, 511]], np.float64)
    grid = np.random.default_rng(4).integers(0, 512, size=(50, 2)).astype(np.float64)
    for k in range(4):
        m = aerial.rigid_matrix(90.0 * k, [0, 0])
        assert (m == np.round(m)).all(), m
        # output corner i reads source corner i + k (the content turns counter-clockwise as displayed: np.rot90's sense)
        np.testing.assert_array_equal(_apply(m, corners), np.roll(corners, -k, axis=0))
        src = _apply(m, grid)
        assert (src == np.round(src)).all() and (src >= 0).all() and (src <= 511).all()
    # the content model: p_new = c + scale R (p_old - c) + shift
    c = np.array([255.5, 255.5])
    a = np.radians(20.0)
    R = np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]])
    m = aerial.rigid_matrix(20.0, [5.0, -9.0], 1.25)
    old = np.array([300.0, 100.0])
    new = c + 1.25 * R @ (old - c) + np.array([5.0, -9.0])
    np.testing.assert_allclose(_apply(m, new), old, atol=1e-10)
    assert abs(m[0] * m[4] - m[1] * m[3]) == pytest.approx(1 / 1.25 ** 2)
    assert aerial.rigid_matrix([0, 90], [0, 0]).shape == (2, 6) and aerial.rigid_matrix(0, [0, 0], [1.0, 2.0]).shape == (2, 6)
    np.testing.assert_allclose(aerial.rigid_matrix(10, [1, 2], centre=(0, 0))[[2, 5]],
                               -np.array([[np.cos(np.radians(10)), -np.sin(np.radians(10))],
                                          [np.sin(np.radians(10)), np.cos(np.radians(10))]]) @ [1, 2], atol=1e-12)
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match="scale"):
            aerial.rigid_matrix(0, [0, 0], bad)
    with pytest.raises(ValueError, match="finite"):
        aerial.rigid_matrix(np.nan, [0, 0])
    with pytest.raises(ValueError, match="rows"):
        aerial.rigid_matrix([0, 1, 2], [[0, 0], [1, 1]])


# ---- KITTI geometry against the Pillow restatement -------------------------------------------------------------------------------
TILE = 1280
# world points (col, row) in tile-1 coordinates, near the tile centre and >= 45 px apart; one brightness level each
WORLD = np.array([[640, 640], [700, 610], [590, 585], [575, 690], [690, 700], [745, 660], [650, 560], [540, 640], [625, 735]])
LEVELS = 255 - 20 * np.arange(len(WORLD))
# (heading rad, gt_shift_x, gt_shift_y, theta) of the two frames, (d col, d row) of the second tile's centre
KITTI_SETS = [
    ((0.30, 0.20, -0.40, 0.50), (0.45, -0.30, 0.10, -0.70), (12, -9)),
    ((0.30, 0.20, -0.40, 0.50), (2.50, 0.60, 0.50, 0.90), (-20, 15)),          # heading difference 126 degrees
    ((0.30, 0.20, -0.40, 0.50), (-2.90, -0.55, -0.65, -1.00), (30, 22)),       # 183 degrees
    ((-1.20, -0.70, 0.30, -0.20), (-1.10, 0.70, -0.30, 0.20), (0, 0)),
    ((-1.20, -0.70, 0.30, -0.20), (0.80, 0.00, 0.00, 0.00), (-31, -18)),       # 115 degrees
    ((-1.20, -0.70, 0.30, -0.20), (1.95, 0.45, 0.75, 1.00), (17, 29)),         # 180 degrees
    ((3.00, 0.10, 0.90, 1.00), (-3.10, -0.10, -0.90, -1.00), (-8, 8)),         # across the +-pi seam
    ((3.00, 0.10, 0.90, 1.00), (1.40, 0.80, -0.20, 0.35), (25, -27)),          # 92 degrees
    ((3.00, 0.10, 0.90, 1.00), (3.00, 0.10, 0.90, 1.00), (9, 4)),              # the same view from a moved tile
]
_RENDERED = {}


def _tile(motion):
    t = np.zeros((TILE, TILE, 1), np.uint8)
    for (cx, cy), level in zip(WORLD - np.asarray(motion), LEVELS):
        t[cy - 2:cy + 3, cx - 2:cx + 3] = level
    return t


def _render(params, motion):
    key = (params, tuple(motion))
    if key not in _RENDERED:
        mats, filters = aerial.kitti_matrices(*params, (TILE, TILE))
        top, left = aerial.center_crop_box(TILE, TILE)
        _RENDERED[key] = (mats[0], pil_warp.crop(pil_warp.chain(_tile(motion), mats[0], filters), top, left, 512, 512)[..., 0])
    return _RENDERED[key]


def _blobs(img):
    """{blob id: weighted centroid (col, row)} of the blobs that lie wholly inside the image"""
    ys, xs = np.nonzero(img)
    seeds, members = [], []
    for y, x in zip(ys, xs):
        for i, (sy, sx) in enumerate(seeds):
            if abs(y - sy) <= 12 and abs(x - sx) <= 12:
                members[i].append((y, x))
                break
        else:
            seeds.append((y, x))
            members.append([(y, x)])
    out = {}
    for pix in members:
        pix = np.array(pix)
        if pix.min() < 2 or pix.max() > 509 or len(pix) < 12:
            continue          # cut by the border of the crop
        w = img[pix[:, 0], pix[:, 1]].astype(np.float64)
        ident = int(np.argmin(np.abs(LEVELS - w.max())))
        assert abs(LEVELS[ident] - w.max()) <= 3 and ident not in out
        out[ident] = (float((w * pix[:, 1]).sum() / w.sum()), float((w * pix[:, 0]).sum() / w.sum()))
    return out


@pytest.mark.parametrize("case", range(len(KITTI_SETS)))
def test_kitti_track_matrix_against_the_pillow_restatement(case):
    prev, nxt, motion = KITTI_SETS[case]
    mats1, crop1 = _render(prev, (0, 0))
    mats2, crop2 = _render(nxt, motion)
    m = aerial.kitti_track_matrix(mats1, mats2, (TILE, TILE), motion)
    assert m.shape == (6,)
    b1, b2 = _blobs(crop1), _blobs(crop2)
    both = sorted(set(b1) & set(b2))
    assert len(both) >= 3, (case, sorted(b1), sorted(b2))
    worst = 0.0
    for ident in both:
        got = _apply(m, b2[ident])
        worst = max(worst, float(np.hypot(*(got - np.array(b1[ident])))))
    print(f"set {case}: {len(both)} blobs in both crops, worst distance {worst:.2f} px")
    assert worst <= 1.5, (case, worst)
    # crop -> tile on its own: the blob's centroid in the crop lands on its world point in the tile
    for mats, blobs, off in ((mats1, b1, (0, 0)), (mats2, b2, motion)):
        to_tile = aerial.kitti_crop_to_tile(mats, (TILE, TILE))
        for ident, centroid in blobs.items():
            assert np.hypot(*(_apply(to_tile, centroid) - (WORLD[ident] - np.asarray(off)))) <= 1.5
    # batched in, batched out
    pair = aerial.kitti_track_matrix(np.stack([mats1, mats1]), np.stack([mats2, mats2]), (TILE, TILE), [motion, motion])
    assert pair.shape == (2, 6)
    np.testing.assert_array_equal(pair[0], m)
    np.testing.assert_array_equal(pair[1], m)


# ---- the crafted stream of the GPU filter test -----------------------------------------------------------------------------------

def test_the_turning_stream_fools_the_argmax_and_not_the_filter():
    """float64 restatement of the filter on the stream tests/track_affine_ref builds: its matrices are aerial.rigid_matrix's, the
    per-frame argmax sits on the distractor in the frames where it is the larger peak, the tracked argmax stays within 2 px of the true
    peak in every frame after the first, and its margin over the runner-up is wide enough for the device to find the same pixel."""
    ref = track_affine_ref
    taps = aerial.gaussian_taps(ref.SEQ_SIGMA, ref.SEQ_RADIUS)
    ori = np.zeros((1, 2, N), np.float32)
    ori[:, 0] = 1.0
    belief = None
    a = np.radians(ref.SEQ_TURN_DEG)
    for k in range(ref.SEQ_FRAMES):
        tx, ty = ref.sequence_truth(k)
        assert 40 <= tx <= 470 and 40 <= ty <= 470 and np.hypot(tx - ref.SEQ_DISTRACTOR[0], ty - ref.SEQ_DISTRACTOR[1]) > 60
        ak = a * k
        step = np.array([[np.cos(ak), np.sin(ak)], [-np.sin(ak), np.cos(ak)]]) @ np.array(ref.SEQ_STEP)
        np.testing.assert_allclose(ref.sequence_matrix(k), aerial.rigid_matrix(ref.SEQ_TURN_DEG, step, centre=ref.SEQ_CENTRE), atol=1e-12)
        lg = ref.sequence_logits(k)[None]
        plain = int(np.argmax(lg[0]))
        on_distractor = track_ref.pixel_distance(plain, ref.SEQ_DISTRACTOR) <= 1.0
        assert on_distractor == (k in ref.SEQ_STRONG), (k, plain)
        if not on_distractor:
            assert track_ref.pixel_distance(plain, (tx, ty)) <= 1.0
        lp = None
        if belief is not None:
            lp = ref.predict(belief, ref.sequence_matrix(k), taps, ref.SEQ_FLOOR).astype(np.float32).reshape(1, N)
        rows, margin, h = track_ref.update(lg, ori, lp)
        if k >= 1:
            assert track_ref.pixel_distance(int(rows[0, 0]), (tx, ty)) <= 2.0, (k, rows[0])
        assert margin[0] > 1e-4, (k, margin)
        belief = h.astype(np.float32).reshape(1, 512, 512)
