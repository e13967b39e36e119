"""Which convolution tile takes which launch, and which split code a request becomes: the documented rules of the four tile families
(kernels.h, conv_tile_runs / conv_tile_splits in kernels_igemm.hip and each family's *_supported) restated in Python for the
kernel-level tests.  The tests derive what they expect from HERE and assert that the library's own answer (requested_runs of
ccvpe_op_conv2d_ex) agrees - a rule that moves in the library shows up as a disagreement, not as a silently different tile."""
from dataclasses import dataclass, field

CONV_TICKETS = 8192            # kernels.h: ticket counters of one launch = output regions a self-reducing split may have
PW_KMAX = 512                  # kernels_pw.hip: deepest K the pointwise slab is staged for
PW_LDS = 150 * 1024            # ... and the LDS bytes slab + four C patches may take
X_WIDTHS = [32, 48, 64, 80, 96, 128]     # conv_wino4x_<width>: the xi-split F(4x4) form takes a layer in ONE n-block of its width
PROJ_CFGS = {(2, 5), (4, 5), (2, 7), (4, 7), (1, 12), (2, 12), (1, 20)}   # kernels_proj.hip: (row tiles, column tiles) instantiated
WINO4_MIN_N = 40               # the packer makes F(4x4) weights for layers of at least 40 output channels


@dataclass
class Launch:
    """One launch as the hook builds it.  N is the GEMM width (4 x cout for a transposed conv), M its rows (input pixels for a
    transposed conv, whose packed form is a 1x1 conv)."""
    B: int
    H: int
    W: int
    Cin: int
    N: int
    K: int = 1                 # kernel edge (the transposed conv is packed as K = 1)
    stride: int = 1
    pad: int = 0
    in_ld: int = 0
    gate: bool = False
    resid: bool = False
    deconv: bool = False
    dsts: list = field(default_factory=list)   # (ld, coff); empty: one dense destination

    def __post_init__(self):
        self.in_ld = self.in_ld or self.Cin
        self.OH = (self.H + 2 * self.pad - self.K) // self.stride + 1
        self.OW = (self.W + 2 * self.pad - self.K) // self.stride + 1
        self.M = self.B * self.OH * self.OW
        self.taps = self.K * self.K
        self.Kpad = -(-self.taps * self.Cin // 32) * 32
        if not self.dsts:
            self.dsts = [(self.N // 4 if self.deconv else self.N, 0)]


def _round16(n):
    return -(-n // 16)


def proj_packed(L):
    """pack_conv makes the fragment-order copy: a gated-project-shaped 1x1 layer (conv_proj_wanted) or a deep-K 1x1 / k2s2 one
    (conv_proj_lat_wanted)."""
    wanted = L.taps == 1 and L.Cin % 16 == 0 and L.Cin >= 192 and _round16(L.N) in (5, 7, 12, 20)
    lat = L.taps * L.Cin >= 480 and L.K in (1, 2)
    return wanted or lat


def _wino_shaped(L):
    return (L.K == 3 and L.stride == 1 and L.pad == 1 and not L.deconv and not L.gate and not L.resid and len(L.dsts) == 1 and
            L.H % 16 == 0 and L.W % 16 == 0 and L.Cin % 8 == 0)


def tile_runs(name, L):
    """(runs, rule): whether tile `name` takes launch L, and the rule that refuses it."""
    if name.startswith("conv_igemm_"):
        return True, ""
    if name.startswith("conv_bf16x3_"):
        return True, ""            # (the hook always packs the bf16 planes)
    if name.startswith("conv_wino4x_"):
        if not _wino_shaped(L):
            return False, "Winograd: 3x3 / stride 1 / pad 1, H and W multiples of 16, no gate, residual or second destination"
        w = int(name.rsplit("_", 1)[1])
        ok = L.N >= 24 and next((x for x in X_WIDTHS if L.N <= x), None) == w
        return ok, "" if ok else f"xi-split tiles serve the layers whose narrowest fitting width they are (24 <= N <= {w})"
    if name.startswith("conv_wino"):
        if not _wino_shaped(L):
            return False, "Winograd: 3x3 / stride 1 / pad 1, H and W multiples of 16, no gate, residual or second destination"
        ld, coff = L.dsts[0]
        if L.N % 4 or ld % 4 or coff % 4:
            return False, "F(2x2) and F(4x4) store 4 channels per lane: N, ld and coff multiples of 4"
        if name.startswith("conv_wino4_") and L.N < WINO4_MIN_N:
            return False, "F(4x4) weights are packed for >= 40 output channels"
        return True, ""
    one = L.K == 1 and L.stride == 1 and L.pad == 0
    if name.startswith("conv_pw_"):
        bn = int(name.rsplit("_", 1)[1])
        if not (one and L.Cin % 4 == 0 and L.in_ld % 4 == 0):
            return False, "pointwise: 1x1 / stride 1 / pad 0"
        if L.Kpad > PW_KMAX:
            return False, f"pointwise: K {L.Kpad} > {PW_KMAX}"
        lds = (bn * (L.Kpad + 4) + 4 * 16 * (bn + 4)) * 4
        return lds <= PW_LDS, f"{name}: slab of {bn} x ({L.Kpad} + 4) floats + C patches = {lds} B exceeds 150 KB"
    if name.startswith("conv_projl_"):
        rt = {"1": 101, "2": 102, "4": 104, "r2": 121, "r4": 141}[name.rsplit("_", 1)[1]]
        k2s2 = L.K == 2 and L.stride == 2 and L.pad == 0 and L.OH * 2 == L.H and L.OW * 2 == L.W and not L.gate and not L.deconv
        if not proj_packed(L):
            return False, "latency form: fragment copy only for K >= 480 (or a gated-project width)"
        if not ((one or k2s2) and L.in_ld % 4 == 0 and L.Cin >= 64 and L.M <= 4096):
            return False, "latency form: 1x1 or k2s2, Cin >= 64, at most 4096 rows"
        if L.gate and L.Cin % 16:
            return False, "latency form with a gate: Cin a multiple of 16"
        if rt == 104 and L.gate:
            return False, "conv_projl_4 refuses a gate (registers)"
        if rt > 104:
            rows = 16 * ((rt - 100) // 10)
            if L.gate or L.M < rows or L.M > 1024:
                return False, f"{name}: no gate, {rows} <= M <= 1024"
        steps = _round16(L.Cin) * L.taps
        return steps <= 16 * 40, "latency form: at most 640 K steps"
    if name.startswith("conv_proj_r"):
        rt = int(name[len("conv_proj_r"):])
        if not L.gate:
            return False, "conv_proj_r*: gated project convs only"
        if not (one and not L.deconv and L.Cin % 16 == 0 and L.in_ld % 4 == 0 and L.Cin >= 64):
            return False, "conv_proj_r*: 1x1, Cin a multiple of 16 and >= 64"
        if not proj_packed(L):
            return False, "conv_proj_r*: fragment copy only for Cin >= 192 and 5 / 7 / 12 / 20 column tiles"
        ok = (rt, _round16(L.N)) in PROJ_CFGS
        return ok, f"conv_proj_r{rt}: no instantiation for {_round16(L.N)} column tiles"
    raise KeyError(name)


def expected_split(name, L, code):
    """The split code launch_conv_igemm and the tile's launcher end up with when tile `name` (which takes L) is asked for `code`
    (S: slabs + reduce launch, 64 + S: self-reducing, 255: F(4x4) tail split) with a slab and ticket counters, and the rule."""
    if code <= 1:
        return 1, ""
    fused = 64 < code <= 96
    S = code - 64 if fused else code
    if name.startswith(("conv_pw_", "conv_proj_r")):
        return 1, "the pointwise persistent and gated-project tiles keep K whole"
    if name.startswith("conv_projl_"):
        rt, ct = {"1": (1, 1), "2": (1, 2), "4": (1, 4), "r2": (2, 1), "r4": (4, 1)}[name.rsplit("_", 1)[1]]
        regions = -(-L.M // (16 * rt)) * -(-_round16(L.N) // ct)
        if not fused or L.gate or regions > CONV_TICKETS:
            return 1, "the latency form splits K only self-reducing, without a gate, within the ticket counters"
        return code, ""
    if code == 255:
        if not name.startswith("conv_wino4_"):
            return 1, "only the F(4x4) tiles have a tail split"
        # kernels_wino4.hip: the work items are whole rounds of the resident workgroups plus a remainder that is a whole number
        # of n-blocks, and that remainder leaves each workgroup room for at least two K slices
        nw, resident = (8, 256) if name.endswith("x128") else (4, 512)
        mblocks, nblocks = L.B * (L.W // 16) * (L.H // 16), -(-_round16(L.N) // nw)
        rem = (mblocks * nblocks) % resident
        tail_nb = rem // mblocks
        ok = rem != 0 and rem % mblocks == 0 and 0 < tail_nb < nblocks and min(resident // rem, _round16(L.Cin) // 2) >= 2
        return (255, "") if ok else (1, "no whole-n-block remainder to split: the launch runs plain")
    if not fused:
        return S, ""
    if name.startswith(("conv_bf16x3_", "conv_wino4x_")):
        return S, "bf16x3 and xi-split tiles do not reduce themselves: slabs + reduce launch"
    if name.startswith("conv_igemm_"):
        bm, bn = (int(v) for v in name.split("_")[2].split("x"))
        regions = -(-L.M // bm) * -(-L.N // bn)
        return (code, "") if regions <= CONV_TICKETS else (S, "more output regions than ticket counters")
    # the persistent Winograd grids: a workgroup's units must fit its ticket list (64)
    resident = max((512 if not name.startswith("conv_wino4_16x128") else 256) // S, 8)
    if name.startswith("conv_wino4_"):
        nw = 8 if name.endswith("x128") else 4
        units = L.B * (L.W // 16) * (L.H // 16) * -(-_round16(L.N) // nw)
        per = -(-units // min(units, resident)) + 8
    else:
        rows, cols = (int(v) for v in name.split("_")[2].split("x"))
        nm = rows // 32
        units = L.B * (L.W // 16) * (L.H // (8 * nm)) * -(-_round16(L.N) // (cols // 16))
        per = -(-units // min(units, max(512 // S, 8))) + 1
    if units > CONV_TICKETS or per > 64:
        return S, "a persistent Winograd workgroup with more units than its ticket list holds"
    return code, ""


WINO_SHAPES = [
    # B, H, W, Cin, Cout
    (1, 16, 16, 8, 16),
    (3, 16, 16, 64, 88),
    (2, 48, 32, 24, 40),
    (1, 32, 48, 104, 17),      # not a multiple of 4 channels: every Winograd tile refuses it
    (1, 32, 48, 104, 20),      # a partly filled last 16-channel slice
    (2, 16, 16, 200, 160),
    (1, 64, 64, 16, 100),
    (1, 32, 32, 48, 32),       # conv2_ori-shaped: the 32-wide xi-split configuration
    (2, 16, 32, 88, 64),       # conv3_ori-shaped (64), Cin = 88: a half-filled last 16-channel group
    (1, 32, 32, 104, 80),      # conv3-shaped: eight waves, 3 + 2 slices
    (1, 16, 16, 24, 30),       # not a multiple of 4 channels: only the xi-split form (one channel per lane in its epilogue) takes it
]

RAN = set()                    # names of the tiles a checked launch of this session was seen to run as requested


def tile_names():
    from ccvpe_amd import _lib
    lib = _lib.load()
    return [lib.ccvpe_op_tile_name(t).decode() for t in range(1, lib.ccvpe_op_num_tiles() + 1)]


def tile_id(name):
    return tile_names().index(name) + 1


def tol_for(name):
    """The suite's bounds, relative to the reference's max: 2e-5 for the fp32 implicit GEMM, the pointwise family and F(2x2);
    1e-4 for bf16x3 (the 3-term split carries ~2^-16 per product) and F(4x4) (transform constants up to 8)."""
    return 1e-4 if ("bf16x3" in name or "wino4" in name) else 2e-5


def run_checked(x, w, b, name, code=0, *, stride=1, pad=0, act=0, gate=None, resid=None, deconv=False, dst_specs=None, what="", record=True):
    """One launch of tile `name` with split code `code` through ccvpe_op_conv2d_ex into pre-filled destinations.  Asserts that
    the library's requested_runs agrees with tile_runs(); that the tile ran as requested with the split expected_split() derives,
    or - refused by rule - that another tile ran; that nothing outside [coff, coff + Cout) of any destination row (and the guard
    row behind the last) was written.  record=False: the launch is not entered in RAN (its caller holds the result to no error bound).  Returns (the [.., Cout] result regions of the destinations, ran_name, ran_split, ran as
    requested)."""
    from ccvpe_amd import _lib
    from tests import conv_ref
    B, H, W, in_ld = x.shape
    if deconv:
        cin, cout = w.shape[0], w.shape[1]
        L = Launch(B, H, W, cin, 4 * cout, 1, 1, 0, in_ld, gate is not None, resid is not None, True, list(dst_specs or []))
        OH, OW = 2 * H, 2 * W
    else:
        cout, cin, K = w.shape[0], w.shape[1], w.shape[2]
        L = Launch(B, H, W, cin, cout, K, stride, pad, in_ld, gate is not None, resid is not None, False, list(dst_specs or []))
        OH, OW = L.OH, L.OW
    bufs = [conv_ref.make_dst(B, OH, OW, ld, x.device) for ld, _ in L.dsts]
    dsts = [(view, coff) for (_, view), (_, coff) in zip(bufs, L.dsts)]
    tid = tile_id(name)
    _, ran, split, runs = _lib.op_conv2d_ex(x, w, b, stride, pad, act, tid | (code << 8), gate=gate, resid=resid, dsts=dsts, deconv=deconv)
    tag = f"{what} tile {name} code {code}"
    want, rule = tile_runs(name, L)
    assert runs == int(want), f"{tag}: the library says runs={runs}, the rule table {want} ({rule})"
    if want:
        assert ran == name, f"{tag}: ran {ran}"
        exp, srule = expected_split(name, L, code)
        assert split == exp, f"{tag}: split code {split}, expected {exp} ({srule})"
        if record:
            RAN.add(name)
    else:
        assert rule and ran != name and ran != "", f"{tag}: refused by rule ({rule}) but ran {ran!r}"
    for (flat, view), (ld, coff) in zip(bufs, L.dsts):
        assert conv_ref.untouched_outside(flat, view, coff, cout), f"{tag}: wrote outside channels [{coff}, {coff + cout}) of a {ld}-wide row"
    return [view[..., coff:coff + cout] for (_, view), (_, coff) in zip(bufs, L.dsts)], ran, split, want
