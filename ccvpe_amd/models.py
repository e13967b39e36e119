"""Host-side mirror of the reference `models` module for the inference path.

Exports the four classes the reference drivers import (train_VIGOR.py:17-18, train_KITTI.py:17,
train_OxfordRobotCar.py:17) with the same constructor arguments, the same 818-key `state_dict`
layout (strict `load_state_dict` of a reference checkpoint succeeds) and the same
`forward(grd, sat) -> 9-tuple` contract (models.py:150, 448, 752, 1051).  The modules own ordinary
torch parameters (so `.to()`, `.eval()`, `.state_dict()` behave), but `forward` does not run a
PyTorch graph: it hands device pointers to libccvpe_hip.so through the C ABI in include/ccvpe.h.

Inference only: no autograd through the HIP path, `eval()` mode required, GPU required.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib, spec, tuning

__all__ = ["CVM_VIGOR", "CVM_VIGOR_ori_prior", "CVM_KITTI", "CVM_OxfordRobotCar"]


# ---------------------------------------------------------------------------------------------
# parameter containers (no forward of their own): they only reproduce the reference key layout
# ---------------------------------------------------------------------------------------------
class _Params(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter container: the forward pass runs in libccvpe_hip.so")


def _bn(c: int) -> nn.BatchNorm2d:
    # momentum = 1 - 0.99, eps 1e-3 (efficientnet_pytorch/model.py:171-172, utils.py:665-666)
    return nn.BatchNorm2d(c, momentum=0.01, eps=spec.BN_EPS)


class _MBConvParams(_Params):
    """Key layout of MBConvBlock (efficientnet_pytorch/model.py:57-87)."""

    def __init__(self, e: int, k: int, s: int, cin: int, cout: int):
        super().__init__()
        mid = cin * e
        if e != 1:
            self._expand_conv = nn.Conv2d(cin, mid, 1, bias=False)
            self._bn0 = _bn(mid)
        self._depthwise_conv = nn.Conv2d(mid, mid, k, stride=s, groups=mid, bias=False)
        self._bn1 = _bn(mid)
        sq = spec.se_squeeze(cin)
        self._se_reduce = nn.Conv2d(mid, sq, 1)
        self._se_expand = nn.Conv2d(sq, mid, 1)
        self._project_conv = nn.Conv2d(mid, cout, 1, bias=False)
        self._bn2 = _bn(cout)


class _EfficientNetParams(_Params):
    """Key layout of EfficientNet-B0 as CCVPE builds it (efficientnet_pytorch/model.py:162-219)."""

    def __init__(self):
        super().__init__()
        self._conv_stem = nn.Conv2d(3, spec.STEM_CH, 3, stride=2, bias=False)
        self._bn0 = _bn(spec.STEM_CH)
        self._blocks = nn.ModuleList([_MBConvParams(*b) for b in spec.B0_BLOCKS])
        self._conv_head = nn.Conv2d(spec.B0_BLOCKS[-1][4], spec.HEAD_CH, 1, bias=False)
        self._bn1 = _bn(spec.HEAD_CH)
        self._fc = nn.Linear(spec.HEAD_CH, spec.FC_CLASSES)   # unused by CCVPE, present in checkpoints


def _double_conv(cin: int, mid: int, cout: int) -> nn.Sequential:
    return nn.Sequential(nn.Conv2d(cin, mid, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(mid, cout, 3, padding=1))


# ---------------------------------------------------------------------------------------------
# the two descriptions a call into the library is built from: where its inputs come from, what it returns
# ---------------------------------------------------------------------------------------------
def _foreign(extra, dev) -> bool:
    """whether a tensor among a form's own arguments (a prior, a table) lives on another device than the inputs"""
    return any(isinstance(a, torch.Tensor) and a.device != dev for a in extra)


class _Layout(tuple):
    """What a call returns: its result slots in the order of the C arguments, each (shape after B, dtype, wanted).  A slot that is not
    wanted - an optional output nobody asked for - is not allocated and goes to the library as a null pointer."""

    def alloc(self, B: int, dev):
        res, ptrs = [], []
        for tail, dtype, wanted in self:       # (a plain loop and plain addresses: a one-launch call is mostly this host time)
            if wanted:
                res.append(torch.empty((B,) + tail, dtype=dtype, device=dev))
                ptrs.append(res[-1].data_ptr())
            else:
                ptrs.append(None)
        return res, ptrs


class _JointResults:
    """The joint filter's results behind _Layout's interface: its slots, with given[i] - a tensor the caller passed as out= - standing
    in for slot i instead of a new one (None: a new one)."""

    def __init__(self, slots, given):
        self.slots, self.given = slots, given

    def alloc(self, B: int, dev):
        res = [self.given.get(i) if self.given.get(i) is not None else torch.empty((B,) + tail, dtype=dtype, device=dev)
               for i, (tail, dtype, _) in enumerate(self.slots)]
        return res, [t.data_ptr() for t in res]


class _NineOutputs:
    """forward's results behind _Layout's interface: the nine tensors, handed over as one ccvpe_outputs struct"""

    def __init__(self, model):
        self.model = model

    def alloc(self, B: int, dev):
        out, res = self.model._alloc_outputs(B, dev)
        return res, (C.byref(out),)


def _slot(*tail, dtype=torch.float32, wanted=True):
    return tail, dtype, bool(wanted)


_MAP = _slot(*spec.OUT_HW)
_ROWS = _Layout((_slot(5),))                       # the argmax forms
_ROWS_MAP = _Layout((_slot(5), _MAP))              # the update forms: rows and their posterior
_ONE_MAP = _Layout((_MAP,))
_SUMMARY = _Layout((_slot(16),))
_POSE_INT = _Layout((_slot(5, dtype=torch.int32),))   # postprocess: the rows as the kernel's integer / float bit patterns


# the layouts that depend on a method's arguments are kept (the last 64 combinations each): a call looks its layout up
@functools.lru_cache(maxsize=64)
def _rows_layout(k: int) -> _Layout:
    return _ROWS if k == 0 else _Layout((_slot(k, 5),))


@functools.lru_cache(maxsize=64)
def _row_layout(n: int) -> _Layout:
    return _Layout((_slot(n),))


@functools.lru_cache(maxsize=64)
def _summary_layout(posterior: bool) -> _Layout:
    return _Layout((_slot(5), _slot(16), _slot(*spec.OUT_HW, wanted=posterior)))


@functools.lru_cache(maxsize=64)
def _heading_layout(bins: int, summary: bool, posterior: bool) -> _Layout:
    return _Layout((_slot(5), _slot(12), _slot(bins), _slot(16, wanted=summary), _slot(*spec.OUT_HW, wanted=posterior)))


@functools.lru_cache(maxsize=64)
def _credible_layout(L: int, level_map: bool, posterior: Optional[bool]) -> _Layout:
    """rows [B, 5] (posterior is None: the stored-map form, which has neither rows nor a posterior), cred [B, 4 + 3 L], then the
    optional level map [B, 512, 512] uint8 and posterior"""
    cred = (_slot(4 + 3 * L), _slot(*spec.OUT_HW, dtype=torch.uint8, wanted=level_map))
    return _Layout(cred if posterior is None else (_slot(5),) + cred + (_slot(*spec.OUT_HW, wanted=posterior),))


class _Images:
    """Input side (grd, sat).  A side checks and normalises its tensors in two steps, check() before the form's own arguments are
    looked at and bind() after, exactly where each check has always stood; t is the tensor that gives B and the device; names picks
    the side's entry of a family's C names; sync: whether the call may have measured a plan (the network runs)."""
    names, sync = 0, True

    def __init__(self, grd, sat):
        self.t, self.sat = grd, sat

    def check(self, m) -> int:
        self.t, self.sat = m._prepare(self.t, self.sat)
        return self.t.shape[0]

    def bind(self, m, name: str, extra):
        g = self.t
        if _foreign(extra, g.device):
            raise ValueError("log_prior must be on the inputs' device")
        return name, (g, g.shape[2], g.shape[3], self.sat)


class _Cached:
    """Input side (grd, cache, tile_index).  ccvpe_<name> takes n_tiles and a nullable tile_index if the name ends in _indexed; the older
    forms have two entry points each, ccvpe_<name> without tile_index (it enforces B <= micro_batch) and ccvpe_<name>_indexed with it."""
    names, sync = 1, True

    def __init__(self, grd, cache, tile_index):
        self.t, self.cache, self.tile_index = grd, cache, tile_index

    def check(self, m) -> int:
        m._require_eval()
        g = self.t
        self.idx = m._host_tile_index(self.tile_index, g)
        if not g.is_cuda or g.dim() != 4 or g.shape[1] != 3:
            raise ValueError("grd must be a cuda tensor [B,3,H,W]")
        return g.shape[0]

    def bind(self, m, name: str, extra):
        if _foreign(extra, self.t.device):
            raise ValueError("log_prior must be on the inputs' device")
        g = self.t = self.t.detach().to(torch.float32).contiguous()
        m._ensure_handle(g.device)
        idx = self.idx
        n_tiles = m._cache_tiles(self.cache, g.shape[0], idx)
        src = (g, g.shape[2], g.shape[3], self.cache.data_ptr())
        if name.endswith("_indexed") or idx is not None:
            name = name if name.endswith("_indexed") else name + "_indexed"
            src += (n_tiles, idx.ctypes.data_as(C.c_void_p) if idx is not None else None)
        return name, src


class _Held:
    """Input side (logits, ori): forward outputs the caller holds.  No network runs, so no plan is built."""
    names, sync = 2, False

    def __init__(self, logits, ori):
        self.t, self.ori = logits, ori

    def check(self, m) -> int:
        m._require_eval()
        logits, ori = self.t, self.ori
        B = logits.shape[0] if logits.dim() > 0 else 0
        if logits.numel() != B * m.PRIOR_MAP or ori.numel() != B * 2 * m.PRIOR_MAP or B == 0:
            raise ValueError(f"expected logits [B,512*512] and ori [B,2,512,512], got {tuple(logits.shape)} / {tuple(ori.shape)}")
        return B

    def bind(self, m, name: str, extra):
        logits, ori = self.t, self.ori
        if not (logits.is_cuda and ori.is_cuda):
            raise RuntimeError("ccvpe_amd has no CPU path: logits and ori must live on an MI355X (cuda) device")
        if logits.device != ori.device or _foreign(extra, logits.device):
            raise ValueError("logits, ori and log_prior must be on one device")
        self.t = logits.detach().to(torch.float32).contiguous()
        ori = ori.detach().to(torch.float32).contiguous()
        m._ensure_handle(self.t.device)
        return name, (self.t, ori)


class _Family:
    """One definition of a family of forms: names = the C names (after ccvpe_) of its image, cached and held-outputs form (None: the
    family has no such form); args(model, B, t, *a) (t: the side's tensor, for a form that needs its device) checks the methods' own arguments a and returns (the C arguments between batch
    and the results, the _Layout); own_first = the sides (their `names`) on which args runs before the inputs' checks - on the
    others it runs after them.  That precedence is behaviour the methods have always had."""

    def __init__(self, names, args, own_first=()):
        self.names, self.args, self.own_first = names, args, own_first


class _JointFilter:
    """The joint position-heading filter's two methods, mixed into _CVMBase: a filter over (heading bin, cell) beside
    the position forms, with a state layout, results and a work buffer of its own."""

    @staticmethod
    def _joint_maps(t, what: str, nb: Optional[int] = None, B: Optional[int] = None):
        """A joint state argument - [B, nb, 512, 512], float32, contiguous, nb in 4..72, B * nb <= 32768 - -> (B, nb); with nb and B
        given it must have exactly that shape.  Where it lives is checked by the caller."""
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what} must be a float32 cuda tensor [B,nb,512,512]")
        shape = tuple(t.shape)
        if len(shape) != 4 or shape[0] < 1 or shape[2:] != spec.OUT_HW:
            raise ValueError(f"{what} must be [B,nb,512,512], got {shape}")
        if nb is not None and shape[:2] != (B, nb):
            raise ValueError(f"{what} must be [{B},{nb},512,512], got {shape}")
        if not 4 <= shape[1] <= 72:
            raise ValueError(f"{what} must hold nb in 4..72 heading bins, got {shape[1]}")
        if shape[0] * shape[1] > 32768:
            raise ValueError(f"{what} holds {shape[0] * shape[1]} maps, at most 32768 per call")
        if t.dtype != torch.float32:
            raise ValueError(f"{what} must be float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{what} must be contiguous")
        return shape[0], shape[1]

    def _joint_work(self, dev, nbytes: int) -> torch.Tensor:
        """the predict's work buffer: one per (device, current stream) - calls on two streams of one model never share one, calls on
        one stream are ordered by it -, grown to the largest size asked for"""
        cache = self.__dict__.setdefault("_joint_work_cache", {})
        key = (dev, torch.cuda.current_stream(dev).cuda_stream)
        buf = cache.get(key)
        if buf is None or buf.numel() < nbytes:
            cache.pop(key, None)
            buf = cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return buf

    def track_joint_predict(self, joint: torch.Tensor, shift_px, taps, floor, turn_deg, heading_taps, out: Optional[torch.Tensor] = None
                            ) -> torch.Tensor:
        """The predict half of a joint filter step: the prior [B, nb, 512, 512] of the next frame from a joint posterior [B, nb, 512,
        512] (track_joint_update_logits' joint).  The map of every SOURCE heading bin k is moved by shift_px[b, k] = (dx, dy) output
        pixels (aerial.joint_shift_table) and blurred with taps as track_predict does; the bins are then turned by turn_deg (a number
        or [B], positive when the heading angle grows) with linear weights, blurred on the circle with heading_taps ([rh+1] or
        [B, rh+1], 2 rh + 1 <= nb), and floor (a number or [B], >= 0) is added: linear values, the definition in include/ccvpe.h
        (ccvpe_track_joint_predict).  Two launches.  out: a [B, nb, 512, 512] tensor to write into, not the joint.  The small
        arguments may be host data or tensors on the joint's device; the work buffer is kept by the model, one per stream."""
        self._require_eval()
        B, nb = self._joint_maps(joint, "joint")
        tshape, stride, radius, number = self._blur_checks(taps, floor, B)
        hshape = tuple(heading_taps.shape) if isinstance(heading_taps, (torch.Tensor, np.ndarray)) else np.shape(heading_taps)
        if len(hshape) not in (1, 2) or hshape[-1] < 1 or (len(hshape) == 2 and hshape[0] != B):
            raise ValueError(f"heading_taps must be [rh+1] or [{B}, rh+1], got {tuple(hshape)}")
        rh = int(hshape[-1]) - 1
        if rh > 32 or 2 * rh + 1 > nb:
            raise ValueError(f"heading_taps give radius {rh}, must be in 0..32 with 2 radius + 1 <= nb = {nb}")
        if out is not None:
            self._joint_maps(out, "out", nb, B)
            if out.data_ptr() == joint.data_ptr():
                raise ValueError("out must not be the joint")
        dev = joint.device
        # shapes and values first (so that they are refused without a device), then the copies
        sh = self._track_vec(shift_px, "shift_px", (B, nb, 2), dev)
        tp = self._track_vec(taps, "taps", tshape, dev)
        ht = self._track_vec(heading_taps, "heading_taps", hshape, dev)
        tn = self._per_query(turn_deg, np.ndim(turn_deg) == 0 and not isinstance(turn_deg, torch.Tensor), "turn_deg", B, dev)
        fl = self._per_query(floor, number, "floor", B, dev)
        if not joint.is_cuda:
            raise ValueError(f"joint must be a cuda tensor, not a {joint.device.type} tensor")
        if out is not None and out.device != dev:
            raise ValueError(f"out is on {out.device}, joint on {dev}")
        self._ensure_handle(dev)
        work = self._joint_work(dev, _lib.load().ccvpe_track_joint_work_bytes(B, nb))
        return self._launch("track_joint_predict", dev, B,
                            (joint, B, nb, sh, tp, stride, radius, tn, ht, (rh + 1) if len(hshape) == 2 else 0, rh, fl, work),
                            _JointResults((_slot(nb, *spec.OUT_HW),), {0: out}))

    def track_joint_predict_affine(self, joint: torch.Tensor, matrix, taps, floor, turn_deg, heading_taps, out: Optional[torch.Tensor] = None
                                   ) -> torch.Tensor:
        """track_joint_predict across frames whose grids differ by more than a translation: the map of every SOURCE
        heading bin k is read through its own affine map matrix[b, k] - OUTPUT pixel index -> SOURCE index position, bilinear
        weights, times |m0 m4 - m1 m3|, as track_predict_affine reads a belief - in place of a shift; the xy blur, the turn of the
        bins, the blur on the circle and the floor are track_joint_predict's (the definition in include/ccvpe.h,
        ccvpe_track_joint_predict_affine).  matrix is [B, nb, 6], or [nb, 6] for one table shared by every query
        (aerial.joint_matrix_table): host data, which must be finite, or a float64 tensor on the joint's device, which is not looked
        at (non-finite entries there may give NaN, never a read outside the joint).  joint, taps, floor, turn_deg, heading_taps and
        out as in track_joint_predict; turn_deg is the change of the heading label between the two grids, the rotation of the grid
        included (aerial.AffineJointTracker adds it).  Two launches, always the affine kernel: the matrices (1, 0, -dx, 0, 1, -dy)
        are track_joint_predict's shifts (dx, dy), bit for bit at integer shifts."""
        self._require_eval()
        B, nb = self._joint_maps(joint, "joint")
        tshape, stride, radius, number = self._blur_checks(taps, floor, B)
        hshape = tuple(heading_taps.shape) if isinstance(heading_taps, (torch.Tensor, np.ndarray)) else np.shape(heading_taps)
        if len(hshape) not in (1, 2) or hshape[-1] < 1 or (len(hshape) == 2 and hshape[0] != B):
            raise ValueError(f"heading_taps must be [rh+1] or [{B}, rh+1], got {tuple(hshape)}")
        rh = int(hshape[-1]) - 1
        if rh > 32 or 2 * rh + 1 > nb:
            raise ValueError(f"heading_taps give radius {rh}, must be in 0..32 with 2 radius + 1 <= nb = {nb}")
        if out is not None:
            self._joint_maps(out, "out", nb, B)
            if out.data_ptr() == joint.data_ptr():
                raise ValueError("out must not be the joint")
        dev = joint.device
        # shapes and values first (so that they are refused without a device), then the copies
        on_device = isinstance(matrix, torch.Tensor) and matrix.device.type != "cpu"
        if on_device:
            mt = matrix.detach()
            if mt.dtype != torch.float64:
                raise ValueError(f"matrix on the device must be float64, got {mt.dtype}")
        else:
            # (a copy: a broadcast table, as aerial.AffineJointTracker passes one, is a read-only view)
            mt = torch.as_tensor(np.array(matrix.detach().numpy() if isinstance(matrix, torch.Tensor) else matrix, dtype=np.float64))
        if tuple(mt.shape) not in ((nb, 6), (B, nb, 6)):
            raise ValueError(f"matrix must be [{nb}, 6] or [{B}, {nb}, 6], got {tuple(mt.shape)}")
        if not on_device and not bool(torch.isfinite(mt).all()):
            raise ValueError("matrix must be finite")
        tp = self._track_vec(taps, "taps", tshape, dev)
        ht = self._track_vec(heading_taps, "heading_taps", hshape, dev)
        tn = self._per_query(turn_deg, np.ndim(turn_deg) == 0 and not isinstance(turn_deg, torch.Tensor), "turn_deg", B, dev)
        fl = self._per_query(floor, number, "floor", B, dev)
        if not joint.is_cuda:
            raise ValueError(f"joint must be a cuda tensor, not a {joint.device.type} tensor")
        if out is not None and out.device != dev:
            raise ValueError(f"out is on {out.device}, joint on {dev}")
        if on_device and mt.device != dev:
            raise ValueError(f"matrix is on {mt.device}, joint on {dev}")
        mt = mt.expand(B, nb, 6).to(dev).contiguous()
        self._ensure_handle(dev)
        work = self._joint_work(dev, _lib.load().ccvpe_track_joint_work_bytes(B, nb))
        return self._launch("track_joint_predict_affine", dev, B,
                            (joint, B, nb, mt, tp, stride, radius, tn, ht, (rh + 1) if len(hshape) == 2 else 0, rh, fl, work),
                            _JointResults((_slot(nb, *spec.OUT_HW),), {0: out}))

    def track_joint_update_logits(self, logits: torch.Tensor, ori: torch.Tensor, emission, prior: Optional[torch.Tensor] = None,
                                  out: Optional[torch.Tensor] = None):
        """The update half of a joint filter step, from forward outputs the caller holds (logits [B, 512*512], ori [B, 2, 512, 512]):
        (rows [B, 5], joint [B, nb, 512, 512], marginal [B, 512, 512], hist [B, nb]).  emission is [nb+1] or [B, nb+1] non-negative
        weights (aerial.heading_emission): entry j < nb weighs a heading j bins ahead of the cell's own, entry nb any heading at a
        cell without one.  prior: track_joint_predict's, or None for the first frame.  joint = logit weight x emission x prior over
        its float64 sum; marginal its sum over the bins - a belief map for belief_summary and belief_credible -, hist its sum over
        the cells, rows aerial.JOINT_FIELDS.  A query without a finite posterior gets the row (-1, NaN, -1, m, Z) and zeros.  out: a
        [B, nb, 512, 512] tensor to write the joint into; it may be the prior (ccvpe_track_joint_update_logits)."""
        self._require_eval()
        side = _Held(logits, ori)
        B = side.check(self)
        on_device = isinstance(emission, torch.Tensor) and emission.device.type != "cpu"
        eshape = tuple(emission.shape) if isinstance(emission, (torch.Tensor, np.ndarray)) else np.shape(emission)
        if len(eshape) not in (1, 2) or (len(eshape) == 2 and eshape[0] != B):
            raise ValueError(f"emission must be [nb+1] or [{B}, nb+1], got {tuple(eshape)}")
        nb = int(eshape[-1]) - 1
        if not 4 <= nb <= 72:
            raise ValueError(f"emission must hold nb + 1 entries with nb in 4..72, got {eshape[-1]}")
        if B * nb > 32768:
            raise ValueError(f"{B} queries of {nb} bins are {B * nb} maps, at most 32768 per call")
        if not on_device:
            ev = np.asarray(emission.detach() if isinstance(emission, torch.Tensor) else emission, dtype=np.float64)
            if not (ev >= 0.0).all():
                raise ValueError("emission must be non-negative (and not NaN)")
        for t, what in ((prior, "prior"), (out, "out")):
            if t is not None:
                self._joint_maps(t, what, nb, B)
        dev = logits.device
        _, (lg, fo) = side.bind(self, "track_joint_update_logits", tuple(t for t in (prior, out) if t is not None))
        em = self._track_vec(emission, "emission", eshape, dev)
        return self._launch("track_joint_update_logits", dev, B, (lg, fo, B, prior, em, (nb + 1) if len(eshape) == 2 else 0, nb),
                            _JointResults((_slot(5), _slot(nb, *spec.OUT_HW), _MAP, _slot(nb)), {1: out}))


class _CVMBase(_JointFilter, nn.Module):
    _variant: str = ""

    def __init__(self, device, circular_padding: bool = False, ori_noise: Optional[float] = None,
                 micro_batch: int = 0, precision: str = "fp32", weight_cache: Optional[str] = None):
        super().__init__()
        v = spec.VARIANTS[self._variant]
        self.device = device
        self.circular_padding = bool(circular_padding)
        self.ori_noise = ori_noise
        self._micro_batch = int(micro_batch)
        if precision not in ("fp32", "bf16x3"):
            raise ValueError("precision must be 'fp32' (exact fp32 MFMA) or 'bf16x3' (3-term bf16 split, ~1e-5 relative)")
        self._precision = precision
        # packed-weight cache directory: None = environment CCVPE_WEIGHT_CACHE, empty = off
        self._weight_cache = weight_cache if weight_cache is not None else os.environ.get("CCVPE_WEIGHT_CACHE", "")
        self.last_weight_source = None   # "packed-cache" or "state_dict" after the first forward (introspection / tests)

        self.grd_efficientnet = _EfficientNetParams()
        for lvl, c in enumerate(v.head_ch, 1):
            setattr(self, f"grd_feature_to_descriptor{lvl}", nn.Sequential(
                nn.Conv2d(spec.HEAD_CH, c, 1), nn.Identity(), nn.Conv2d(v.feat_h, 1, 1), nn.Flatten(start_dim=1)))
        self.sat_efficientnet = _EfficientNetParams()
        self.sat_feature_to_descriptors = nn.Sequential(nn.Flatten(start_dim=1), nn.Linear(spec.HEAD_CH * 4, v.sat_desc))
        for sfx, dec in (("", v.loc), ("_ori", v.ori)):
            for j, lv in enumerate(dec):
                n = 6 - j
                setattr(self, f"deconv{n}{sfx}", nn.ConvTranspose2d(lv.deconv_in, lv.deconv_out, 2, 2))
                setattr(self, f"conv{n}{sfx}", _double_conv(lv.deconv_out + lv.skip, lv.mid, lv.out))

        self._handle: Optional[C.c_void_p] = None
        self._handle_device: Optional[int] = None
        self._weights_dirty = True
        self._debug = False
        self._rolls: Tuple[int, ...] = ()

    # ---- lifetime of the native handle ------------------------------------------------------
    def _release(self):
        if getattr(self, "_handle", None) is not None:
            try:
                _lib.load().ccvpe_destroy(self._handle)
            finally:
                self._handle = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _apply(self, fn, *a, **k):       # .to() / .cuda() / .cpu() move the parameters
        out = super()._apply(fn, *a, **k)
        self._weights_dirty = True
        return out

    def load_state_dict(self, state_dict, strict: bool = True, *a, **k):
        out = super().load_state_dict(state_dict, strict, *a, **k)
        self._weights_dirty = True
        return out

    def refresh_weights(self) -> None:
        """Call after modifying parameters in place: the next forward re-ingests the state_dict."""
        self._weights_dirty = True

    def _ensure_handle(self, dev: torch.device) -> None:
        lib = _lib.load()
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        if self._handle is not None and self._handle_device != index:
            self._release()
        if self._handle is None:
            cfg = _lib.Config()
            cfg.variant = _lib.VARIANT_ID[self._variant]
            cfg.circular_padding = int(self.circular_padding)
            cfg.ori_noise = float(self.ori_noise) if self.ori_noise is not None else 0.0
            cfg.device = index
            cfg.micro_batch = self._micro_batch
            cfg.reserved[0] = 1 if self._precision == "bf16x3" else 0
            h = C.c_void_p()
            _lib.check(lib.ccvpe_create(C.byref(cfg), C.byref(h)), "ccvpe_create")
            self._handle, self._handle_device = h, index
            self._weights_dirty = True
            self._rolls = tuple(lib.ccvpe_output_channels(h, k) for k in range(6))
            tuning.load_into(lib, h)     # committed table + this machine's cache: known plans are not measured again
            self._tune_gen = lib.ccvpe_tuning_generation(h)
            if self._debug:
                _lib.check(lib.ccvpe_set_debug(h, 1), "ccvpe_set_debug")
            if getattr(self, "_n_streams", 2) != 2:
                _lib.check(lib.ccvpe_set_streams(h, self._n_streams), "ccvpe_set_streams")
        if self._weights_dirty:
            sd = self.state_dict()
            cache_file = self._cache_path(sd) if self._weight_cache else None
            if cache_file and os.path.exists(cache_file) and lib.ccvpe_load_packed(self._handle, cache_file.encode()) == 0:
                self.last_weight_source = "packed-cache"
            else:
                for key, t in sd.items():
                    if t.dtype != torch.float32 or "._fc." in key:
                        _lib.check(lib.ccvpe_skip_weight(self._handle, key.encode()), f"ccvpe_skip_weight({key})")
                        continue
                    t = t.detach().contiguous()
                    shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
                    _lib.check(lib.ccvpe_set_weight(self._handle, key.encode(), C.c_void_p(t.data_ptr()), shape, t.dim()),
                               f"ccvpe_set_weight({key})")
                if dev.type == "cuda":
                    torch.cuda.synchronize(dev)
                _lib.check(lib.ccvpe_finalize_weights(self._handle), "ccvpe_finalize_weights")
                self.last_weight_source = "state_dict"
                if cache_file:   # best effort: a lost race or a read-only directory costs the re-pack on the next start only
                    try:
                        os.makedirs(os.path.dirname(cache_file), exist_ok=True)
                        if lib.ccvpe_save_packed(self._handle, cache_file.encode()) != 0:
                            import warnings
                            warnings.warn(f"ccvpe_amd: packed-weight cache not written: {(lib.ccvpe_last_error() or b'').decode()}")
                    except OSError as e:
                        import warnings
                        warnings.warn(f"ccvpe_amd: packed-weight cache not written: {e}")
            self._weights_dirty = False

    def _tuning_sync(self) -> None:
        """After a call that may have built a plan: write the tuning table back when this handle has measured a new one."""
        gen = _lib.load().ccvpe_tuning_generation(self._handle)
        if gen != getattr(self, "_tune_gen", 0):
            self._tune_gen = gen
            tuning.save_from(_lib.load(), self._handle)

    def export_tuning(self) -> str:
        """Text of this handle's tuning table (plans loaded at start plus plans measured since)."""
        return tuning.export(_lib.load(), self._handle) if self._handle is not None else ""

    def _cache_path(self, sd) -> str:
        """File name of the packed weights of this exact state dict: content hash of every float tensor in key order,
        variant, precision, padding mode and the digest of the library sources (a rebuilt library repacks)."""
        import hashlib
        try:
            import xxhash
            hsh = xxhash.xxh3_128()
        except ImportError:
            hsh = hashlib.sha256()
        for key in sorted(sd):
            t = sd[key]
            if t.dtype != torch.float32 or "._fc." in key:
                continue
            hsh.update(key.encode())
            hsh.update(t.detach().cpu().contiguous().numpy().tobytes())
        # switches that change what the packer emits are part of the key, and so is the library actually loaded
        sw = _lib.load().ccvpe_pack_switches() or b""   # the library's own list: whatever its packer branches on
        if sw:
            hsh.update(sw)
        tag = f"{self._variant}-{self._precision}-{int(self.circular_padding)}-{_lib.library_digest()[:16]}-{hsh.hexdigest()[:32]}"
        return os.path.join(self._weight_cache, tag + ".ccvpepack")

    # ---- forward ----------------------------------------------------------------------------
    def _prepare(self, grd: torch.Tensor, sat: torch.Tensor):
        if self.training:
            raise RuntimeError("ccvpe_amd runs the inference path only: call .eval() first "
                               "(reference test loops do, train_VIGOR.py:254)")
        if not (grd.is_cuda and sat.is_cuda):
            raise RuntimeError("ccvpe_amd has no CPU path: inputs must live on an MI355X (cuda) device")
        if grd.device != sat.device:
            raise RuntimeError("grd and sat must be on the same device")
        if grd.dim() != 4 or sat.dim() != 4 or grd.shape[1] != 3 or sat.shape[1] != 3 or grd.shape[0] != sat.shape[0]:
            raise ValueError(f"expected grd [B,3,H,W] and sat [B,3,512,512], got {tuple(grd.shape)} / {tuple(sat.shape)}")
        if tuple(sat.shape[2:]) != spec.SAT_HW:
            raise ValueError(f"aerial input must be 3x512x512, got {tuple(sat.shape)}")
        grd = grd.detach().to(torch.float32).contiguous()
        sat = sat.detach().to(torch.float32).contiguous()
        self._ensure_handle(grd.device)
        return grd, sat

    def _alloc_outputs(self, B: int, dev: torch.device):
        n = spec.OUT_HW[0] * spec.OUT_HW[1]
        logits = torch.empty((B, n), dtype=torch.float32, device=dev)
        heat = torch.empty((B, 1) + spec.OUT_HW, dtype=torch.float32, device=dev)
        ori = torch.empty((B, 2) + spec.OUT_HW, dtype=torch.float32, device=dev)
        ms = [torch.empty((B, self._rolls[k], 8 << k, 8 << k), dtype=torch.float32, device=dev) for k in range(6)]
        out = _lib.Outputs()
        out.logits_flattened = logits.data_ptr()
        out.heatmap = heat.data_ptr()
        out.ori = ori.data_ptr()
        for k in range(6):
            out.matching_score[k] = ms[k].data_ptr()
        return out, (logits, heat, ori, *ms)

    def _require_eval(self) -> None:
        if self.training:
            raise RuntimeError("ccvpe_amd runs the inference path only: call .eval() first")

    def _launch(self, name: str, dev, B: int, cargs, layout, sync: bool = False):
        """Every call with results enters the library here, behind its checks and _ensure_handle: allocate the layout's tensors, call
        ccvpe_<name>(handle, *cargs, *result pointers, stream) under dev on its current stream, check the return code, sync the tuning
        table if the call may have built a plan.  cargs: tensors go by address (the bindings declare every pointer a void pointer, which
        takes an integer), None as a null pointer.  Returns the results in the layout's order: a tuple, or the tensor itself when
        there is one."""
        name = "ccvpe_" + name
        with torch.cuda.device(dev):
            res, ptrs = layout.alloc(B, dev)
            cargs = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in cargs]
            rc = getattr(_lib.load(), name)(self._handle, *cargs, *ptrs, torch.cuda.current_stream(dev).cuda_stream)
        if rc != _lib.OK:
            _lib.check(rc, name)
        if sync:
            self._tuning_sync()
        return res[0] if len(res) == 1 else tuple(res)

    def _run(self, family: _Family, side, *a):
        """The skeleton of forward and every pose form: the side checks its inputs, the family its own arguments a - before them on the
        sides the family names in own_first, else after -, the side normalises its tensors and ensures the handle, and the call goes
        out through _launch with the C arguments (side's, batch, family's)."""
        own = side.names in family.own_first
        if own:
            self._require_eval()
            made = family.args(self, side.t.shape[0], side.t, *a)   # (before the inputs' checks)
        B = side.check(self)
        extra, layout = made if own else family.args(self, B, side.t, *a)
        name, src = side.bind(self, family.names[side.names], extra)
        return self._launch(name, side.t.device, B, src + (B,) + tuple(extra), layout, side.sync)

    _FORWARD = _Family(("forward", "forward_cached", None), lambda self, B, t: ((), _NineOutputs(self)))
    _LOCALIZE = _Family(("localize", "localize_cached", None), lambda self, B, t: ((), _ROWS))

    def forward(self, grd: torch.Tensor, sat: torch.Tensor):
        return self._run(self._FORWARD, _Images(grd, sat))

    # ---- aerial-side caching for streaming -------------------------------
    def encode_aerial(self, sat: torch.Tensor) -> torch.Tensor:
        """Encode aerial images once; the returned device buffer feeds forward_cached() for any number of
        ground frames that share the tile (Oxford RobotCar reuses tiles, datasets.py:306-317)."""
        self._require_eval()
        if not sat.is_cuda or sat.dim() != 4 or tuple(sat.shape[1:]) != (3,) + spec.SAT_HW:
            raise ValueError("sat must be a cuda tensor [B,3,512,512]")
        return self._encode("aerial", sat)

    def _encode(self, side: str, img: torch.Tensor, hw=()) -> torch.Tensor:
        """encode_aerial / encode_ground behind their input checks: the cache of ccvpe_<side>_cache_bytes, written by ccvpe_encode_<side>
        (hw: the image size, an argument of the ground side only), with the image count recorded on it."""
        img = img.detach().to(torch.float32).contiguous()
        self._ensure_handle(img.device)
        lib = _lib.load()
        B = img.shape[0]
        nbytes = getattr(lib, f"ccvpe_{side}_cache_bytes")(self._handle, B, *hw)
        cache = torch.empty(nbytes // 4, dtype=torch.float32, device=img.device)
        stream = torch.cuda.current_stream(img.device).cuda_stream
        _lib.check(getattr(lib, f"ccvpe_encode_{side}")(self._handle, C.c_void_p(img.data_ptr()), *hw, B, C.c_void_p(cache.data_ptr()),
                                                         C.c_void_p(stream)), f"ccvpe_encode_{side}")
        self._tuning_sync()
        cache._ccvpe_batch = B
        return cache

    @staticmethod
    def _host_tile_index(tile_index, grd: torch.Tensor) -> Optional[np.ndarray]:
        """tile_index keyword of the cached calls -> contiguous host int32 [B] (None stays None).  Host data only: a device tensor is
        refused rather than copied back, which would hide a synchronisation.  Range checks are the library's (ccvpe_*_indexed)."""
        if tile_index is None:
            return None
        if isinstance(tile_index, torch.Tensor):
            if tile_index.device.type != "cpu":
                raise ValueError(f"tile_index is host data: pass a CPU tensor, a numpy array or a sequence, not a {tile_index.device.type} "
                                 "tensor (copying it back would synchronise)")
            tile_index = tile_index.numpy()
        idx = np.asarray(tile_index)
        B = grd.shape[0] if grd.dim() > 0 else -1
        if idx.shape != (B,):
            raise ValueError(f"tile_index must hold one tile per query: shape ({B},) expected, got {idx.shape}")
        if B > 0 and not np.issubdtype(idx.dtype, np.integer):
            raise ValueError(f"tile_index must hold integers, got {idx.dtype}")
        i32 = np.ascontiguousarray(idx, dtype=np.int32)
        if not np.array_equal(i32, idx):
            raise ValueError("tile_index entries must fit in int32")
        return i32

    @staticmethod
    def _cache_tiles(cache: torch.Tensor, B: int, idx: Optional[np.ndarray]) -> int:
        """Tiles a cached call's cache holds: B for the unindexed calls (which need exactly one per query), else the count
        encode_aerial recorded."""
        if idx is None:
            if getattr(cache, "_ccvpe_batch", B) != B:
                raise ValueError("cache was encoded for a different batch size")
            return B
        if not hasattr(cache, "_ccvpe_batch"):
            raise ValueError("tile_index needs a cache returned by encode_aerial (it records how many tiles the cache holds)")
        return int(cache._ccvpe_batch)

    def forward_cached(self, grd: torch.Tensor, cache: torch.Tensor, tile_index=None):
        """forward(grd, sat) with the aerial side taken from encode_aerial(sat).  tile_index (host ints [B], optional): query b
        reads tile tile_index[b] of a cache encode_aerial wrote for any number of tiles up to the micro-batch, and B may then
        be any size (ccvpe_forward_cached_indexed)."""
        return self._run(self._FORWARD, _Cached(grd, cache, tile_index))

    # ---- one ground encoding against several aerial tiles ---------------------------------------
    def encode_ground(self, grd: torch.Tensor) -> torch.Tensor:
        """Encode ground images once: the returned device buffer (float32 [B * Ltot], the descriptor vector of each image, layout in
        include/ccvpe.h) feeds localize_region, which pairs each image with several aerial tiles (ccvpe_encode_ground)."""
        self._require_eval()
        if not grd.is_cuda or grd.dim() != 4 or grd.shape[1] != 3:
            raise ValueError("grd must be a cuda tensor [B,3,H,W]")
        self._ensure_handle(grd.device)
        B, H, W = grd.shape[0], grd.shape[2], grd.shape[3]
        if _lib.load().ccvpe_ground_cache_bytes(self._handle, B, H, W) == 0:   # (a size the variant does not take)
            _lib.check(-1, "ccvpe_ground_cache_bytes")
        cache = self._encode("ground", grd, (H, W))
        cache._ccvpe_grd_hw = (H, W)
        return cache

    @staticmethod
    def _host_region_tiles(tiles):
        """tiles argument of localize_region -> (offsets int32 [G+1], flat int32 [P]) on the host.  Host data only, as tile_index of
        the cached calls: device tensors are refused.  Range checks against the cache are the library's (ccvpe_localize_region)."""
        def host(v, what):
            if isinstance(v, torch.Tensor):
                if v.device.type != "cpu":
                    raise ValueError(f"{what} is host data: pass CPU tensors, numpy arrays or sequences, not a {v.device.type} tensor "
                                     "(copying it back would synchronise)")
                return v.numpy()
            return v
        tiles = host(tiles, "tiles")
        if isinstance(tiles, (str, bytes)) or not hasattr(tiles, "__len__"):
            raise ValueError("tiles must be a sequence of per-query tile-id sequences")
        if len(tiles) == 0:
            raise ValueError("tiles must name at least one query")
        offsets = [0]
        flat = []
        for g, t in enumerate(tiles):
            a = np.asarray(host(t, "tiles"))
            if a.ndim != 1:
                raise ValueError(f"tiles[{g}] must be a 1-D sequence of tile ids, got shape {a.shape}")
            if a.shape[0] == 0:
                raise ValueError(f"tiles[{g}] is empty: every query needs at least one tile")
            if not np.issubdtype(a.dtype, np.integer) or a.dtype == np.bool_:
                raise ValueError(f"tiles[{g}] must hold integers, got {a.dtype}")
            if (a < 0).any():
                raise ValueError(f"tiles[{g}] holds a negative tile id {int(a[a < 0][0])}")
            i32 = a.astype(np.int32)
            if not np.array_equal(i32, a):
                raise ValueError(f"tiles[{g}] entries must fit in int32")
            flat.append(i32)
            offsets.append(offsets[-1] + a.shape[0])
        if offsets[-1] > np.iinfo(np.int32).max:
            raise ValueError("too many (query, tile) pairs for int32 offsets")
        return np.ascontiguousarray(offsets, dtype=np.int32), np.ascontiguousarray(np.concatenate(flat), dtype=np.int32)

    def localize_region(self, ground_cache: torch.Tensor, sat_cache: torch.Tensor, tiles) -> Dict[str, object]:
        """Every query of encode_ground(grd) against its own list of tiles of encode_aerial(sat): tiles[g] = the tile ids of query g
        (host ints, a ragged sequence of G sequences; ids may repeat).  Returns, on the device unless noted:
            rows [G,5]       (index, prob, cos, sin, angle_deg) of the query's best pair, prob = the softmax over the union of its
                             tiles at that pair's argmax;
            pair [G] int32   the position of that pair in the flattened pair list;
            pair_tile        host int32 [P], the tile of each pair (pair_tile[pair[g]] is query g's chosen tile);
            pair_rows [P,5]  localize rows of each pair, the probability inside its tile;
            pair_stats [P,2] (max logit, 1 / sum exp) of each pair's softmax;
            tile_prob [P]    each pair's share of its query's summed softmax mass (ccvpe_localize_region)."""
        return self._region(ground_cache, sat_cache, tiles)

    _NO_PRIOR = object()   # (not None: localize_region_prior refuses a None prior as it refuses any other non-tensor)

    def _region(self, ground_cache, sat_cache, tiles, pair_log_prior=_NO_PRIOR) -> Dict[str, object]:
        """localize_region and, with a pair_log_prior, localize_region_prior."""
        prior = pair_log_prior is not self._NO_PRIOR
        self._require_eval()
        offsets, flat = self._host_region_tiles(tiles)
        G, P = offsets.shape[0] - 1, flat.shape[0]
        if prior:
            lp, stride, _, _ = self._prior_args(pair_log_prior, P, 0, 0)
        for what, c in (("ground_cache", ground_cache), ("sat_cache", sat_cache)):
            if not isinstance(c, torch.Tensor) or not c.is_cuda:
                raise ValueError(f"{what} must be the cuda tensor encode_{'ground' if what == 'ground_cache' else 'aerial'} returned")
        if not hasattr(ground_cache, "_ccvpe_grd_hw"):
            raise ValueError("ground_cache must come from encode_ground (it records the image count and size)")
        if not hasattr(sat_cache, "_ccvpe_batch"):
            raise ValueError("sat_cache must come from encode_aerial (it records how many tiles the cache holds)")
        if int(ground_cache._ccvpe_batch) != G:
            raise ValueError(f"tiles names {G} queries, ground_cache holds {ground_cache._ccvpe_batch}")
        if prior and lp.device != ground_cache.device:
            raise ValueError("pair_log_prior must be on the caches' device")
        self._ensure_handle(ground_cache.device)
        dev = ground_cache.device
        H, W = ground_cache._ccvpe_grd_hw
        rows = torch.empty((G, 5), dtype=torch.float32, device=dev)
        pair = torch.empty((G,), dtype=torch.int32, device=dev)
        pair_rows = torch.empty((P, 5), dtype=torch.float32, device=dev)
        pair_stats = torch.empty((P, 2), dtype=torch.float32, device=dev)
        tile_prob = torch.empty((P,), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        name = "ccvpe_localize_region_prior" if prior else "ccvpe_localize_region"
        rc = getattr(_lib.load(), name)(self._handle, C.c_void_p(ground_cache.data_ptr()), G, H, W, C.c_void_p(sat_cache.data_ptr()),
                                        int(sat_cache._ccvpe_batch), offsets.ctypes.data_as(C.c_void_p), flat.ctypes.data_as(C.c_void_p),
                                        *((C.c_void_p(lp.data_ptr()), stride) if prior else ()), C.c_void_p(rows.data_ptr()),
                                        C.c_void_p(pair.data_ptr()), C.c_void_p(pair_rows.data_ptr()), C.c_void_p(pair_stats.data_ptr()),
                                        C.c_void_p(tile_prob.data_ptr()), C.c_void_p(stream))
        _lib.check(rc, name)
        self._tuning_sync()
        return {"rows": rows, "pair": pair, "pair_tile": flat, "pair_rows": pair_rows, "pair_stats": pair_stats, "tile_prob": tile_prob}

    # ---- pose-only forward -------------------------------------------------------------------
    def localize(self, grd: torch.Tensor, sat: torch.Tensor) -> torch.Tensor:
        """The pose of every query without the nine forward outputs: float32 [B, 5] on the device, the postprocess_rows layout
        (index, prob, cos, sin, angle_deg).  Bit-identical to postprocess_rows(*forward(grd, sat)[1:3]), also for a query without a
        finite posterior (one NaN or +inf logit: the heatmap is all NaN), whose row is (-1, NaN, cos, sin, angle_deg of pixel 0) in
        both (ccvpe_localize)."""
        return self._run(self._LOCALIZE, _Images(grd, sat))

    def localize_cached(self, grd: torch.Tensor, cache: torch.Tensor, tile_index=None) -> torch.Tensor:
        """localize(grd, sat) with the aerial side taken from encode_aerial(sat): float32 [B, 5] rows (index, prob, cos, sin,
        angle_deg), the postprocess_rows layout (ccvpe_localize_cached).  tile_index: as forward_cached
        (ccvpe_localize_cached_indexed)."""
        return self._run(self._LOCALIZE, _Cached(grd, cache, tile_index))

    # ---- several pose hypotheses per query ----------------------------------------------------
    @staticmethod
    def _topk_args(k: int, radius: int):
        k, radius = int(k), int(radius)
        if not 1 <= k <= 64:
            raise ValueError(f"k must be in 1..64, got {k}")
        if not 0 <= radius <= 32:
            raise ValueError(f"radius must be in 0..32, got {radius}")
        return k, radius

    def _topk_form(self, B: int, t, k, radius):
        k, radius = self._topk_args(k, radius)
        return (k, radius), _rows_layout(k)

    _TOPK = _Family(("localize_topk", "localize_topk_cached", None), _topk_form)

    def localize_topk(self, grd: torch.Tensor, sat: torch.Tensor, k: int, radius: int) -> torch.Tensor:
        """The k strongest heatmap peaks of every query under a suppression radius, with their orientation: float32 [B, k, 5]
        on the device, rows (index, prob, cos, sin, angle_deg); (-1, 0, 0, 0, 0) past a query's last peak.  Bit-identical to
        postprocess_topk(*forward(grd, sat)[1:3], k, radius) (ccvpe_localize_topk)."""
        return self._run(self._TOPK, _Images(grd, sat), k, radius)

    def localize_topk_cached(self, grd: torch.Tensor, cache: torch.Tensor, k: int, radius: int, tile_index=None) -> torch.Tensor:
        """localize_topk(grd, sat, k, radius) with the aerial side taken from encode_aerial(sat): float32 [B, k, 5]
        (ccvpe_localize_topk_cached).  tile_index: as forward_cached (ccvpe_localize_topk_cached_indexed)."""
        return self._run(self._TOPK, _Cached(grd, cache, tile_index), k, radius)

    def postprocess_topk(self, heatmap: torch.Tensor, ori: torch.Tensor, k: int, radius: int) -> torch.Tensor:
        """postprocess_rows() generalised to the k strongest peaks under a suppression radius, on forward outputs the caller
        holds: float32 [B, k, 5] on the device (ccvpe_postprocess_topk, the definition in include/ccvpe.h)."""
        self._require_eval()
        if not (heatmap.is_cuda and ori.is_cuda):
            raise RuntimeError("ccvpe_amd has no CPU path: heatmap and ori must live on an MI355X (cuda) device")
        k, radius = self._topk_args(k, radius)
        B = heatmap.shape[0]
        if heatmap.numel() != B * 512 * 512 or ori.numel() != B * 2 * 512 * 512:
            raise ValueError(f"expected heatmap [B,1,512,512] and ori [B,2,512,512], got {tuple(heatmap.shape)} / {tuple(ori.shape)}")
        heatmap = heatmap.detach().to(torch.float32).contiguous()
        ori = ori.detach().to(torch.float32).contiguous()
        self._ensure_handle(heatmap.device)
        return self._launch("postprocess_topk", heatmap.device, B, (heatmap, ori, B, k, radius), _rows_layout(k))

    # ---- pose with a position prior -------------------------------------------
    PRIOR_MAP = 512 * 512

    @classmethod
    def _prior_args(cls, log_prior, B: int, k: int, radius: int):
        """(log_prior, k, radius) of the prior forms -> (contiguous float32 cuda tensor, prior_stride in floats, k, radius).  log_prior is
        one map for every query ([512,512], [1,512,512], [1,1,512,512]: stride 0) or one per query ([B,512,512], [B,1,512,512]: stride
        512*512), log-weights in the pixel order of logits_flattened; k = 0 is the argmax form and takes radius 0."""
        k, radius = int(k), int(radius)
        if not 0 <= k <= 64:
            raise ValueError(f"k must be in 0..64 (0: the argmax row), got {k}")
        if not 0 <= radius <= 32:
            raise ValueError(f"radius must be in 0..32, got {radius}")
        if k == 0 and radius != 0:
            raise ValueError(f"radius {radius} needs k >= 1: the argmax form (k = 0) takes radius 0")
        if not isinstance(log_prior, torch.Tensor):
            raise ValueError("log_prior must be a float32 cuda tensor")
        shape = tuple(log_prior.shape)
        ok = shape[-2:] == spec.OUT_HW and (len(shape) in (2, 3) or (len(shape) == 4 and shape[1] == 1))
        n = 1 if len(shape) == 2 else (shape[0] if ok else -1)
        if not ok or n not in (1, B):
            raise ValueError(f"log_prior must be [512,512], [1,512,512], [{B},512,512] or the [.,1,512,512] forms, got {shape}")
        if log_prior.dtype != torch.float32:
            raise ValueError(f"log_prior must be float32, got {log_prior.dtype}")
        if not log_prior.is_contiguous():
            raise ValueError("log_prior must be contiguous")
        if not log_prior.is_cuda:
            raise ValueError(f"log_prior must be a cuda tensor on the inputs' device, not a {log_prior.device.type} tensor")
        return log_prior.detach(), (cls.PRIOR_MAP if n > 1 else 0), k, radius

    def _prior_form(self, B: int, t, log_prior, k, radius):
        a = self._prior_args(log_prior, B, k, radius)
        return a, _rows_layout(a[2])

    _PRIOR = _Family(("localize_prior", "localize_prior_cached_indexed", "postprocess_prior"), _prior_form, own_first=(_Images.names,))

    def localize_prior(self, grd: torch.Tensor, sat: torch.Tensor, log_prior: torch.Tensor, k: int = 0, radius: int = 0) -> torch.Tensor:
        """localize (k = 0: rows [B, 5]) or localize_topk (k in 1..64: rows [B, k, 5]) on the posterior softmax(logits + log_prior):
        the semantics in include/ccvpe.h (ccvpe_localize_prior).  An all-zero prior gives the rows of the forms without one; a query
        without a finite posterior (a prior of -inf everywhere) has index -1."""
        return self._run(self._PRIOR, _Images(grd, sat), log_prior, k, radius)

    def localize_prior_cached(self, grd: torch.Tensor, cache: torch.Tensor, log_prior: torch.Tensor, k: int = 0, radius: int = 0,
                              tile_index=None) -> torch.Tensor:
        """localize_prior(grd, sat, log_prior, k, radius) with the aerial side taken from encode_aerial(sat); tile_index as
        forward_cached (ccvpe_localize_prior_cached_indexed)."""
        return self._run(self._PRIOR, _Cached(grd, cache, tile_index), log_prior, k, radius)

    def postprocess_prior(self, logits: torch.Tensor, ori: torch.Tensor, log_prior: torch.Tensor, k: int = 0, radius: int = 0
                          ) -> torch.Tensor:
        """The rows of localize_prior from forward outputs the caller holds: logits = forward(...)[0] ([B, 512*512]), ori =
        forward(...)[2] ([B, 2, 512, 512]); bit-identical to the pose-only forms (ccvpe_postprocess_prior)."""
        return self._run(self._PRIOR, _Held(logits, ori), log_prior, k, radius)

    def localize_region_prior(self, ground_cache: torch.Tensor, sat_cache: torch.Tensor, tiles, pair_log_prior: torch.Tensor
                              ) -> Dict[str, object]:
        """localize_region with a log-prior per (query, tile) pair: pair_log_prior is one map for every pair or [P,512,512] in the
        flattened pair order (query by query, each query's tiles in order), each map on one scale across a query's tiles - a
        log-density at every heatmap pixel's map position, such as aerial.oxford_log_prior.  Returns localize_region's dict, every
        value of the posterior (ccvpe_localize_region_prior)."""
        return self._region(ground_cache, sat_cache, tiles, pair_log_prior)

    # ---- tracking a frame stream ----------------------------------------------
    @classmethod
    def _track_prior(cls, log_prior, B: int):
        """log_prior of the update forms -> (tensor or None, prior_stride): None means no prior, anything else is checked as
        localize_prior checks it."""
        if log_prior is None:
            return None, 0
        lp, stride, _, _ = cls._prior_args(log_prior, B, 0, 0)
        return lp, stride

    _UPDATE = _Family(("track_update", "track_update_cached_indexed", "track_update_logits"),
                      lambda self, B, t, log_prior: (self._track_prior(log_prior, B), _ROWS_MAP), own_first=(_Images.names,))

    def track_update(self, grd: torch.Tensor, sat: torch.Tensor, log_prior: Optional[torch.Tensor] = None):
        """The update half of a filter step: (rows [B, 5], posterior [B, 512, 512]).  rows are localize_prior(grd, sat, log_prior)'s,
        posterior is the map they are the argmax of - softmax(logits + log_prior) in the pixel order of the logits, with the bits of
        rows[b, 1] at rows[b, 0]; log_prior=None: the forward's heatmap.  A query without a finite posterior gets the row (-1, NaN, ..)
        and an all-zero map (ccvpe_track_update)."""
        return self._run(self._UPDATE, _Images(grd, sat), log_prior)

    def track_update_cached(self, grd: torch.Tensor, cache: torch.Tensor, log_prior: Optional[torch.Tensor] = None, tile_index=None):
        """track_update(grd, sat, log_prior) with the aerial side taken from encode_aerial(sat); tile_index as forward_cached
        (ccvpe_track_update_cached_indexed)."""
        return self._run(self._UPDATE, _Cached(grd, cache, tile_index), log_prior)

    def track_update_logits(self, logits: torch.Tensor, ori: torch.Tensor, log_prior: Optional[torch.Tensor] = None):
        """track_update from forward outputs the caller holds: logits = forward(...)[0] ([B, 512*512]), ori = forward(...)[2]
        ([B, 2, 512, 512]); bit-identical to the pose-only forms (ccvpe_track_update_logits)."""
        return self._run(self._UPDATE, _Held(logits, ori), log_prior)

    @staticmethod
    def _track_vec(value, what: str, shape, dev):
        """A small per-query argument of track_predict -> contiguous float32 tensor of `shape` on dev.  Host data (numbers, sequences,
        numpy arrays, CPU tensors) is copied up; a tensor already on the device is used as it is (no synchronisation either way)."""
        if isinstance(value, torch.Tensor):
            t = value.detach()
            if t.dtype != torch.float32:
                if t.is_floating_point() or t.device.type == "cpu":
                    t = t.to(torch.float32)
                else:
                    raise ValueError(f"{what} must hold floats, got {t.dtype}")
        else:
            t = torch.as_tensor(np.asarray(value, dtype=np.float32))
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what} must have shape {tuple(shape)}, got {tuple(t.shape)}")
        return t.to(dev).contiguous()

    @staticmethod
    def _stored_maps(t, what: str = "belief") -> int:
        """A stored map argument - [B,512,512] or [B,1,512,512], float32, contiguous, at most 4096 maps - -> B.  Where it lives is
        checked by the caller: that check stands at another place in every method."""
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what} must be a float32 cuda tensor [B,512,512]")
        shape = tuple(t.shape)
        if not (len(shape) == 3 and shape[0] >= 1 and shape[1:] == spec.OUT_HW) and not (len(shape) == 4 and shape[0] >= 1 and shape[1] == 1
                                                                                       and shape[2:] == spec.OUT_HW):
            raise ValueError(f"{what} must be [B,512,512] or [B,1,512,512], got {shape}")
        if t.dtype != torch.float32:
            raise ValueError(f"{what} must be float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{what} must be contiguous")
        if shape[0] > 4096:
            raise ValueError(f"{what} holds {shape[0]} maps, at most 4096 per call")
        return shape[0]

    @staticmethod
    def _blur_checks(taps, floor, B: int, nb: Optional[int] = None):
        """The taps, radius and floor checks of the predict methods, in their order -> (taps' shape, taps_stride, radius, whether floor
        is one number; per-query floors are the library's to read).  nb: heading_predict's bin count, which bounds the radius as well
        and has its own sentence for it."""
        tshape = tuple(taps.shape) if isinstance(taps, (torch.Tensor, np.ndarray)) else np.shape(taps)
        if len(tshape) not in (1, 2) or tshape[-1] < 1 or (len(tshape) == 2 and tshape[0] != B):
            raise ValueError(f"taps must be [radius+1] or [{B}, radius+1], got {tuple(tshape)}")
        radius = int(tshape[-1]) - 1
        if nb is None and radius > 32:
            raise ValueError(f"taps give radius {radius}, must be in 0..32")
        if nb is not None and (radius > 32 or 2 * radius + 1 > nb):
            raise ValueError(f"taps give radius {radius}, must be in 0..32 with 2 radius + 1 <= nb = {nb}")
        number = np.ndim(floor) == 0 and not isinstance(floor, torch.Tensor)
        if number and not float(floor) >= 0.0:
            raise ValueError(f"floor must be >= 0, got {floor}")
        return tshape, (radius + 1) if len(tshape) == 2 else 0, radius, number

    @classmethod
    def _per_query(cls, value, number: bool, what: str, B: int, dev):
        """a number or [B] -> float32 [B] on dev"""
        if number:
            return torch.full((B,), float(value), dtype=torch.float32, device=dev)
        return cls._track_vec(value, what, (B,), dev)

    def track_predict(self, belief: torch.Tensor, shift_px, taps, floor) -> torch.Tensor:
        """The predict half of a filter step: the log-prior [B, 512, 512] of the next frame from a posterior map.  belief [B,512,512]
        (track_update's map) is extended by zero, moved by shift_px [B,2] = (dx, dy) output pixels with bilinear weights, blurred
        along x and y with the one-sided taps t[0..radius] ([radius+1] for every query or [B, radius+1]; aerial.gaussian_taps), and
        the result is log(. + floor), floor a number or [B], >= 0: the definition in include/ccvpe.h (ccvpe_track_predict).  One
        launch.  shift_px, taps and floor may be host data or tensors on the belief's device."""
        self._require_eval()
        B = self._stored_maps(belief)
        tshape, stride, radius, number = self._blur_checks(taps, floor, B)
        dev = belief.device
        # shapes and values first (so that they are refused without a device), then the copies
        sh = self._track_vec(shift_px, "shift_px", (B, 2), dev)
        tp = self._track_vec(taps, "taps", tshape, dev)
        fl = self._per_query(floor, number, "floor", B, dev)
        if not belief.is_cuda:
            raise ValueError(f"belief must be a cuda tensor, not a {belief.device.type} tensor")
        self._ensure_handle(dev)
        return self._launch("track_predict", dev, B, (belief, B, sh, tp, stride, radius, fl), _ONE_MAP)

    def track_predict_affine(self, belief: torch.Tensor, matrix, taps, floor) -> torch.Tensor:
        """track_predict under an affine map per query: output pixel index (x, y) reads the belief, extended by zero,
        at index position (m0 x + m1 y + m2, m3 x + m4 y + m5) with bilinear weights, times |m0 m4 - m1 m3|; then the blur, the floor
        and the logarithm of track_predict (the definition in include/ccvpe.h, ccvpe_track_predict_affine).  matrix is [B,6] or [6]
        (one map for every query), OUTPUT index -> SOURCE index position (aerial.rigid_matrix, aerial.kitti_track_matrix;
        aerial.affine_index_form converts a Pillow-convention matrix): host data, which must be finite, or a float64 tensor on the
        belief's device, which is not looked at (non-finite entries there may give NaN, never a read outside the belief).  belief,
        taps and floor as in track_predict.  One launch, always the affine kernel: (1, 0, -dx, 0, 1, -dy) is track_predict's shift
        (dx, dy), bit for bit at integer shifts."""
        self._require_eval()
        B = self._stored_maps(belief)
        on_device = isinstance(matrix, torch.Tensor) and matrix.device.type != "cpu"
        if on_device:
            mt = matrix.detach()
            if mt.dtype != torch.float64:
                raise ValueError(f"matrix on the device must be float64, got {mt.dtype}")
        else:
            mt = torch.as_tensor(np.asarray(matrix.detach() if isinstance(matrix, torch.Tensor) else matrix, dtype=np.float64))
        if tuple(mt.shape) not in ((6,), (B, 6)):
            raise ValueError(f"matrix must be [6] or [{B}, 6], got {tuple(mt.shape)}")
        if not on_device and not bool(torch.isfinite(mt).all()):
            raise ValueError("matrix must be finite")
        tshape, stride, radius, number = self._blur_checks(taps, floor, B)
        dev = belief.device
        # shapes and values first (so that they are refused without a device), then the copies
        tp = self._track_vec(taps, "taps", tshape, dev)
        fl = self._per_query(floor, number, "floor", B, dev)
        if not belief.is_cuda:
            raise ValueError(f"belief must be a cuda tensor, not a {belief.device.type} tensor")
        if on_device and mt.device != dev:
            raise ValueError(f"matrix is on {mt.device}, belief on {dev}")
        mt = mt.expand(B, 6).to(dev).contiguous()
        self._ensure_handle(dev)
        return self._launch("track_predict_affine", dev, B, (belief, B, mt, tp, stride, radius, fl), _ONE_MAP)

    # ---- posterior summary ------------------------------------------------------
    @classmethod
    def _summary_args(cls, log_prior, B: int, radius):
        """(log_prior, radius) of the summary forms -> (tensor or None, prior_stride, radius): the prior as the update forms take it,
        the window radius in 0..32."""
        radius = int(radius)
        if not 0 <= radius <= 32:
            raise ValueError(f"radius must be in 0..32, got {radius}")
        return cls._track_prior(log_prior, B) + (radius,)

    def _summary_form(self, B: int, t, log_prior, radius, posterior):
        return self._summary_args(log_prior, B, radius), _summary_layout(bool(posterior))

    _SUMMARY_FORMS = _Family(("localize_summary", "localize_summary_cached_indexed", "postprocess_summary"), _summary_form,
                             own_first=(_Images.names,))

    def localize_summary(self, grd: torch.Tensor, sat: torch.Tensor, log_prior: Optional[torch.Tensor] = None, radius: int = 8,
                         posterior: bool = False):
        """The pose and how sure it is: (rows [B, 5], summary [B, 16]), with the posterior [B, 512, 512] behind them if asked.  rows
        and posterior are track_update(grd, sat, log_prior)'s; summary holds, per query, the columns aerial.SUMMARY_FIELDS of that
        map - argmax and its value, total mass, entropy, mean and covariance, and the mass, mean and covariance of the
        (2 radius + 1)^2 window around the argmax - in cells of the 512 grid (aerial.summary_to_metres scales them).  No launch is
        added to localize_prior's.  A query without a finite posterior has the summary (-1, NaN, NaN ...) (ccvpe_localize_summary)."""
        return self._run(self._SUMMARY_FORMS, _Images(grd, sat), log_prior, radius, posterior)

    def localize_summary_cached(self, grd: torch.Tensor, cache: torch.Tensor, log_prior: Optional[torch.Tensor] = None, radius: int = 8,
                                posterior: bool = False, tile_index=None):
        """localize_summary(grd, sat, log_prior, radius, posterior) with the aerial side taken from encode_aerial(sat); tile_index as
        forward_cached (ccvpe_localize_summary_cached_indexed)."""
        return self._run(self._SUMMARY_FORMS, _Cached(grd, cache, tile_index), log_prior, radius, posterior)

    def postprocess_summary(self, logits: torch.Tensor, ori: torch.Tensor, log_prior: Optional[torch.Tensor] = None, radius: int = 8,
                            posterior: bool = False):
        """localize_summary from forward outputs the caller holds: logits = forward(...)[0] ([B, 512*512]), ori = forward(...)[2]
        ([B, 2, 512, 512]); bit-identical to the pose-only forms (ccvpe_postprocess_summary)."""
        return self._run(self._SUMMARY_FORMS, _Held(logits, ori), log_prior, radius, posterior)

    def belief_summary(self, belief: torch.Tensor, radius: int = 8) -> torch.Tensor:
        """The summary [B, 16] of stored maps: belief [B,512,512] or [B,1,512,512], float32, contiguous, non-negative - a forward's
        heatmap, a tracker belief; it need not sum to 1 (column 2 is its sum).  An all-zero map gives (0, 0, 0, NaN ...); NaN never
        wins the argmax, and a map without a value above -inf gives index 0 with the map's value there.  One launch
        (ccvpe_belief_summary)."""
        self._require_eval()
        B = self._stored_maps(belief)
        radius = int(radius)
        if not 0 <= radius <= 32:
            raise ValueError(f"radius must be in 0..32, got {radius}")
        if not belief.is_cuda:
            raise ValueError(f"belief must be a cuda tensor, not a {belief.device.type} tensor")
        dev = belief.device
        self._ensure_handle(dev)
        return self._launch("belief_summary", dev, B, (belief, B, radius), _SUMMARY)

    # ---- credible regions -------------------------------------------------------
    @staticmethod
    def _credible_levels(levels) -> np.ndarray:
        """levels of the credible forms -> contiguous host float32 [L], 1 <= L <= 8, each finite and in (0, 1]; any order, repeats allowed"""
        lv = np.ascontiguousarray(np.atleast_1d(np.asarray(levels, dtype=np.float32)))
        if lv.ndim != 1 or not 1 <= lv.size <= 8:
            raise ValueError(f"levels must hold 1..8 numbers, got shape {lv.shape}")
        if not (np.isfinite(lv) & (lv > 0) & (lv <= 1)).all():
            raise ValueError(f"every level must be finite and in (0, 1], got {lv.tolist()}")
        return lv

    @staticmethod
    def _credible_probe(probe, B: int, dev) -> Optional[torch.Tensor]:
        """probe of the credible forms -> None or an int32 tensor [B] on dev: one cell index per query, any value (an index outside
        the map gives NaN and is never dereferenced)"""
        if probe is None:
            return None
        t = probe if isinstance(probe, torch.Tensor) else torch.as_tensor(np.asarray(probe, dtype=np.int64))
        if t.dim() != 1 or t.shape[0] != B or t.is_floating_point():
            raise ValueError(f"probe must hold one integer cell index per query ([{B}]), got {tuple(t.shape)} {t.dtype}")
        return t.detach().clamp(-1, 1 << 30).to(device=dev, dtype=torch.int32).contiguous()

    def _credible_form(self, B: int, t, lv: np.ndarray, log_prior, probe, level_map, posterior):
        """lv: the levels as _credible_levels returns them - the methods convert them before anything else is checked, the image form
        behind its eval guard"""
        extra = self._track_prior(log_prior, B) + (lv.ctypes.data_as(C.c_void_p), int(lv.size), self._credible_probe(probe, B, t.device))
        return extra, _credible_layout(int(lv.size), bool(level_map), bool(posterior))

    _CREDIBLE = _Family(("localize_credible", "localize_credible_cached_indexed", "postprocess_credible"), _credible_form,
                        own_first=(_Images.names,))

    def belief_credible(self, belief: torch.Tensor, levels, probe=None, level_map: bool = False):
        """Credible regions of stored maps: cred [B, 4 + 3 L] for the L levels (each in (0, 1]; any order) - per query the columns
        aerial.CREDIBLE_HEAD_FIELDS (total mass, positive cells, and for the probe cell the mass share and count of the cells strictly
        above it), then aerial.CREDIBLE_LEVEL_FIELDS per level: the threshold value, the region's cells and its share of the mass.
        The region of a level is the smallest set of whole value classes holding that share (include/ccvpe.h has the definition).
        belief as belief_summary takes it; probe: one cell index per query (a tensor or a sequence) or None; level_map=True also
        returns a uint8 map [B, 512, 512] of the number of levels whose region holds each cell: (cred, level_map).  An all-zero
        map gives the level columns (NaN, 0, NaN) (ccvpe_belief_credible)."""
        self._require_eval()
        B = self._stored_maps(belief)
        lv = self._credible_levels(levels)
        if not belief.is_cuda:
            raise ValueError(f"belief must be a cuda tensor, not a {belief.device.type} tensor")
        dev = belief.device
        pr = self._credible_probe(probe, B, dev)
        self._ensure_handle(dev)
        return self._launch("belief_credible", dev, B, (belief, B, lv.ctypes.data_as(C.c_void_p), int(lv.size), pr),
                            _credible_layout(int(lv.size), bool(level_map), None))

    def localize_credible(self, grd: torch.Tensor, sat: torch.Tensor, levels, log_prior: Optional[torch.Tensor] = None, probe=None,
                          level_map: bool = False, posterior: bool = False):
        """The pose and the credible regions of its posterior: (rows [B, 5], cred [B, 4 + 3 L]), then the level map and the posterior
        if asked.  rows and posterior are track_update(grd, sat, log_prior)'s; cred and the level map are belief_credible's on that
        posterior, bit for bit, whether or not it is returned (ccvpe_localize_credible)."""
        self._require_eval()
        return self._run(self._CREDIBLE, _Images(grd, sat), self._credible_levels(levels), log_prior, probe, level_map, posterior)

    def localize_credible_cached(self, grd: torch.Tensor, cache: torch.Tensor, levels, log_prior: Optional[torch.Tensor] = None, probe=None,
                                 level_map: bool = False, posterior: bool = False, tile_index=None):
        """localize_credible with the aerial side taken from encode_aerial(sat); tile_index as forward_cached
        (ccvpe_localize_credible_cached_indexed)."""
        return self._run(self._CREDIBLE, _Cached(grd, cache, tile_index), self._credible_levels(levels), log_prior, probe, level_map,
                         posterior)

    def postprocess_credible(self, logits: torch.Tensor, ori: torch.Tensor, levels, log_prior: Optional[torch.Tensor] = None, probe=None,
                             level_map: bool = False, posterior: bool = False):
        """localize_credible from forward outputs the caller holds: logits = forward(...)[0] ([B, 512*512]), ori = forward(...)[2]
        ([B, 2, 512, 512]); bit-identical to the pose-only forms (ccvpe_postprocess_credible)."""
        return self._run(self._CREDIBLE, _Held(logits, ori), self._credible_levels(levels), log_prior, probe, level_map, posterior)

    # ---- heading posterior ------------------------------------------------------
    @classmethod
    def _heading_args(cls, log_prior, B: int, radius, bins):
        """(log_prior, radius, bins) of the heading forms -> (tensor or None, prior_stride, radius, bins): the prior and the window radius
        as the summary forms take them, the bin count in 4..360."""
        bins = int(bins)
        if not 4 <= bins <= 360:
            raise ValueError(f"bins must be in 4..360, got {bins}")
        return cls._summary_args(log_prior, B, radius) + (bins,)

    @classmethod
    def _window_bins(cls, radius, bins):
        """(radius, bins) of a heading form, checked on their own: the cached and the held-outputs form refuse them before anything
        else - before the eval guard, too -, as they always have"""
        return cls._heading_args(None, 1, radius, bins)[2:]

    def _heading_form(self, B: int, t, log_prior, radius, bins, summary, posterior):
        a = self._heading_args(log_prior, B, radius, bins)
        return a, _heading_layout(a[3], bool(summary), bool(posterior))

    _HEADING = _Family(("localize_heading", "localize_heading_cached_indexed", "postprocess_heading"), _heading_form,
                       own_first=(_Images.names,))

    def localize_heading(self, grd: torch.Tensor, sat: torch.Tensor, log_prior: Optional[torch.Tensor] = None, radius: int = 8,
                         bins: int = 72, summary: bool = False, posterior: bool = False):
        """The pose and the heading the network believes in: (rows [B, 5], heading [B, 12], hist [B, bins]), with the summary [B, 16]
        and the posterior [B, 512, 512] behind them if asked.  rows, summary and posterior are localize_summary(grd, sat, log_prior,
        radius)'s; hist is the posterior's mass per heading bin of 360 / bins degrees (aerial.heading_bin_centres), heading holds the
        columns aerial.HEADING_FIELDS - mass with a heading, mean cos and sin, mean heading, resultant length, mode bin and its
        share, and the same over the (2 radius + 1)^2 window around the argmax.  Computes the whole orientation field and adds one
        launch to localize_prior's.  A query without a finite posterior has heading NaN with mode -1 and an all-zero hist
        (ccvpe_localize_heading)."""
        return self._run(self._HEADING, _Images(grd, sat), log_prior, radius, bins, summary, posterior)

    def localize_heading_cached(self, grd: torch.Tensor, cache: torch.Tensor, log_prior: Optional[torch.Tensor] = None, radius: int = 8,
                                bins: int = 72, summary: bool = False, posterior: bool = False, tile_index=None):
        """localize_heading(grd, sat, log_prior, radius, bins, summary, posterior) with the aerial side taken from encode_aerial(sat);
        tile_index as forward_cached (ccvpe_localize_heading_cached_indexed)."""
        return self._run(self._HEADING, _Cached(grd, cache, tile_index), log_prior, *self._window_bins(radius, bins), summary, posterior)

    def postprocess_heading(self, logits: torch.Tensor, ori: torch.Tensor, log_prior: Optional[torch.Tensor] = None, radius: int = 8,
                            bins: int = 72, summary: bool = False, posterior: bool = False):
        """localize_heading from forward outputs the caller holds: logits = forward(...)[0] ([B, 512*512]), ori = forward(...)[2]
        ([B, 2, 512, 512]); bit-identical to the pose-only forms (ccvpe_postprocess_heading)."""
        return self._run(self._HEADING, _Held(logits, ori), log_prior, *self._window_bins(radius, bins), summary, posterior)

    # ---- heading prior ------------------------------------------------------------
    @staticmethod
    def _hprior_table(table, B: int):
        """heading_log_prior of the heading-prior forms -> (contiguous float32 tensor, table_stride, nb): [nb+1] (one table for every
        query: stride 0) or [B, nb+1] (stride nb + 1) log-weights, nb in 4..360; entry nb is the weight of a cell without a heading."""
        if not isinstance(table, torch.Tensor):
            raise ValueError("heading_log_prior must be a float32 cuda tensor [nb+1] or [B, nb+1]")
        shape = tuple(table.shape)
        if len(shape) not in (1, 2) or (len(shape) == 2 and shape[0] != B):
            raise ValueError(f"heading_log_prior must be [nb+1] or [{B}, nb+1], got {shape}")
        nb = shape[-1] - 1
        if not 4 <= nb <= 360:
            raise ValueError(f"heading_log_prior must hold nb + 1 entries with nb in 4..360, got {shape[-1]}")
        if table.dtype != torch.float32:
            raise ValueError(f"heading_log_prior must be float32, got {table.dtype}")
        if not table.is_contiguous():
            raise ValueError("heading_log_prior must be contiguous")
        if not table.is_cuda:
            raise ValueError(f"heading_log_prior must be a cuda tensor on the inputs' device, not a {table.device.type} tensor")
        return table.detach(), (nb + 1 if len(shape) == 2 else 0), nb

    @classmethod
    def _heading_prior_args(cls, table, log_prior, B: int, radius, bins):
        """The C arguments of the heading-prior forms between batch and the results: (log_prior or None, prior_stride, table,
        table_stride, nb, radius, bins)."""
        lp, stride, radius, bins = cls._heading_args(log_prior, B, radius, bins)
        return (lp, stride) + cls._hprior_table(table, B) + (radius, bins)

    def _heading_prior_form(self, B: int, t, table, log_prior, radius, bins, summary, posterior):
        a = self._heading_prior_args(table, log_prior, B, radius, bins)
        return a, _heading_layout(a[6], bool(summary), bool(posterior))

    _HEADING_PRIOR = _Family(("localize_heading_prior", "localize_heading_prior_cached_indexed", None), _heading_prior_form,
                             own_first=(_Images.names, _Cached.names))   # (this family's cached form, too)

    def heading_prior_map(self, ori: torch.Tensor, heading_log_prior: torch.Tensor, log_prior: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The combined prior map [B, 512, 512] of a heading prior and an optional position prior, from a forward's ori
        ([B, 2, 512, 512]): per cell heading_log_prior[bin of the cell's heading], entry nb for a cell without one, plus log_prior
        there.  heading_log_prior is [nb+1] or [B, nb+1] (aerial.von_mises_heading_log_prior, heading_predict).  The map is the
        log_prior of any prior form - postprocess_prior, postprocess_summary, postprocess_heading, track_update_logits.  One launch
        (ccvpe_heading_prior_map)."""
        self._require_eval()
        if not isinstance(ori, torch.Tensor) or ori.dim() != 4 or ori.shape[0] < 1 or tuple(ori.shape[1:]) != (2,) + spec.OUT_HW:
            raise ValueError(f"ori must be [B,2,512,512], got {tuple(ori.shape) if isinstance(ori, torch.Tensor) else type(ori)}")
        B = ori.shape[0]
        if B > 4096:
            raise ValueError(f"ori holds {B} fields, at most 4096 per call")
        lp, stride = self._track_prior(log_prior, B)
        tb, tstride, nb = self._hprior_table(heading_log_prior, B)
        if not ori.is_cuda:
            raise RuntimeError("ccvpe_amd has no CPU path: ori must live on an MI355X (cuda) device")
        if tb.device != ori.device or (lp is not None and lp.device != ori.device):
            raise ValueError("ori, heading_log_prior and log_prior must be on one device")
        ori = ori.detach().to(torch.float32).contiguous()
        self._ensure_handle(ori.device)
        return self._launch("heading_prior_map", ori.device, B, (ori, B, lp, stride, tb, tstride, nb), _ONE_MAP)

    def localize_heading_prior(self, grd: torch.Tensor, sat: torch.Tensor, heading_log_prior: torch.Tensor,
                               log_prior: Optional[torch.Tensor] = None, radius: int = 8, bins: int = 72, summary: bool = False,
                               posterior: bool = False):
        """localize_heading under a heading prior: what localize_heading(grd, sat, comb, radius, bins, summary, posterior) returns for
        comb = heading_prior_map(ori, heading_log_prior, log_prior), without the detour through the full forward's outputs - bit for
        bit.  heading_log_prior [nb+1] or [B, nb+1]; nb is independent of bins.  One launch more than localize_heading; the carried
        heading belief is treated as independent of the position (ccvpe_localize_heading_prior)."""
        return self._run(self._HEADING_PRIOR, _Images(grd, sat), heading_log_prior, log_prior, radius, bins, summary, posterior)

    def localize_heading_prior_cached(self, grd: torch.Tensor, cache: torch.Tensor, heading_log_prior: torch.Tensor,
                                      log_prior: Optional[torch.Tensor] = None, radius: int = 8, bins: int = 72, summary: bool = False,
                                      posterior: bool = False, tile_index=None):
        """localize_heading_prior with the aerial side taken from encode_aerial(sat); tile_index as forward_cached
        (ccvpe_localize_heading_prior_cached_indexed)."""
        return self._run(self._HEADING_PRIOR, _Cached(grd, cache, tile_index), heading_log_prior, log_prior, radius, bins, summary,
                         posterior)

    def heading_predict(self, hist: torch.Tensor, turn_deg, taps, floor) -> torch.Tensor:
        """The predict half of a filter step on the heading axis: the heading prior [B, nb+1] of the next frame from a hist [B, nb]
        (localize_heading's).  hist is turned by turn_deg (a number or [B]: the heading change since that frame, positive when the
        heading angle grows) with linear weights between the two source bins, blurred on the circle with the one-sided taps
        t[0..radius] ([radius+1] or [B, radius+1]; aerial.gaussian_taps, 2 radius + 1 <= nb), and the result is log(. + floor), floor a
        number or [B], >= 0; the last entry, for a cell without a heading, is what the average bin gets: the definition in
        include/ccvpe.h (ccvpe_heading_predict).  One launch.  turn_deg, taps and floor may be host data or tensors on hist's device."""
        self._require_eval()
        if not isinstance(hist, torch.Tensor) or hist.dim() != 2 or hist.shape[0] < 1:
            raise ValueError("hist must be a float32 cuda tensor [B, nb]")
        B, nb = int(hist.shape[0]), int(hist.shape[1])
        if not 4 <= nb <= 360:
            raise ValueError(f"hist must hold nb in 4..360 bins, got {nb}")
        if hist.dtype != torch.float32:
            raise ValueError(f"hist must be float32, got {hist.dtype}")
        if not hist.is_contiguous():
            raise ValueError("hist must be contiguous")
        if B > 4096:
            raise ValueError(f"hist holds {B} rows, at most 4096 per call")
        tshape, stride, radius, number = self._blur_checks(taps, floor, B, nb)
        dev = hist.device
        # shapes and values first (so that they are refused without a device), then the copies
        tp = self._track_vec(taps, "taps", tshape, dev)
        tn = self._per_query(turn_deg, np.ndim(turn_deg) == 0 and not isinstance(turn_deg, torch.Tensor), "turn_deg", B, dev)
        fl = self._per_query(floor, number, "floor", B, dev)
        if not hist.is_cuda:
            raise ValueError(f"hist must be a cuda tensor, not a {hist.device.type} tensor")
        self._ensure_handle(dev)
        return self._launch("heading_predict", dev, B, (hist, B, nb, tn, tp, stride, radius, fl), _row_layout(nb + 1))

    # ---- extras beyond the reference surface ------------------------------------------------
    def postprocess(self, heatmap: torch.Tensor, ori: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Device-side version of the per-sample loop in train_VIGOR.py:297-316.  The argmax is the largest value above -inf, the first
        index on ties; NaN never wins (numpy.argmax returns the first NaN).  A map without such a value - all NaN, which one NaN or
        +inf logit makes of the softmax, all -inf, a mix - gives index -1, prob NaN and the orientation of pixel 0."""
        B = heatmap.shape[0]
        self._ensure_handle(heatmap.device)
        buf = self._launch("postprocess", heatmap.device, B, (heatmap.contiguous(), ori.contiguous(), B), _POSE_INT)
        f = buf.view(torch.float32)
        return {"index": buf[:, 0].to(torch.int64), "prob": f[:, 1], "cos": f[:, 2], "sin": f[:, 3], "angle_deg": f[:, 4]}

    def postprocess_rows(self, heatmap: torch.Tensor, ori: torch.Tensor) -> torch.Tensor:
        """postprocess() as ONE float32 tensor [B, 5] = (index, prob, cos, sin, angle_deg): the 20-byte rows a data-parallel
        evaluation gathers, written by the post-processing launch itself (no conversion / stack launches behind it).  A map without a
        value above -inf: (-1, NaN, cos, sin, angle_deg of pixel 0), as postprocess()."""
        B = heatmap.shape[0]
        self._ensure_handle(heatmap.device)
        return self._launch("postprocess_rows", heatmap.device, B, (heatmap.contiguous(), ori.contiguous(), B), _ROWS)

    METRIC_FIELDS = ("pixel_distance", "meter_distance", "prob_at_gt", "angle_pred_deg", "angle_gt_deg", "orientation_error_deg",
                     "longitudinal_m", "lateral_m")

    def evaluate(self, heatmap: torch.Tensor, ori: torch.Tensor, gt_index, meter_per_pixel, gt_cos_sin=None, heading_deg=None
                 ) -> Dict[str, torch.Tensor]:
        """Device-side version of the whole per-sample test loop (train_VIGOR.py:290-326, train_KITTI.py:309-343): argmax /
        orientation lookup (postprocess) plus the ground-truth side - pixel and metre distance, probability at the
        ground-truth pixel, orientation error, lateral / longitudinal split.  Returns float64 tensors [B] (NaN where the
        reference produces no value for the query).  A query without an argmax (index -1, see postprocess) has NaN distances; a
        gt_index outside the map has prob_at_gt NaN."""
        B = heatmap.shape[0]
        dev = heatmap.device
        self._ensure_handle(dev)
        heatmap = heatmap.contiguous()
        pose = torch.empty((B, 5), dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        lib = _lib.load()
        _lib.check(lib.ccvpe_postprocess(self._handle, C.c_void_p(heatmap.data_ptr()), C.c_void_p(ori.contiguous().data_ptr()), B,
                                         C.c_void_p(pose.data_ptr()), C.c_void_p(stream)), "ccvpe_postprocess")
        gi = torch.as_tensor(gt_index, dtype=torch.int32, device=dev).contiguous()
        mpp = torch.as_tensor(meter_per_pixel, dtype=torch.float64, device=dev).expand(B).contiguous()
        gcs = None if gt_cos_sin is None else torch.as_tensor(gt_cos_sin, dtype=torch.float32, device=dev).reshape(B, 2).contiguous()
        hd = None if heading_deg is None else torch.as_tensor(heading_deg, dtype=torch.float64, device=dev).expand(B).contiguous()
        out = torch.empty((B, len(self.METRIC_FIELDS)), dtype=torch.float64, device=dev)
        _lib.check(lib.ccvpe_eval_metrics(self._handle, C.c_void_p(pose.data_ptr()), C.c_void_p(heatmap.data_ptr()), B, C.c_void_p(gi.data_ptr()),
                                          C.c_void_p(gcs.data_ptr()) if gcs is not None else None, C.c_void_p(mpp.data_ptr()),
                                          C.c_void_p(hd.data_ptr()) if hd is not None else None, C.c_void_p(out.data_ptr()), C.c_void_p(stream)),
                   "ccvpe_eval_metrics")
        res = {k: out[:, i] for i, k in enumerate(self.METRIC_FIELDS)}
        res["index"] = pose[:, 0].to(torch.int64)
        return res

    def set_streams(self, n: int) -> None:
        """Issue order of later forwards: 2 (default) two-stream schedule, 1 program order (bit-identical results)."""
        self._n_streams = int(n)
        if self._handle is not None:
            _lib.check(_lib.load().ccvpe_set_streams(self._handle, int(n)), "ccvpe_set_streams")

    def set_debug(self, enable: bool) -> None:
        self._debug = bool(enable)
        if self._handle is not None:
            _lib.check(_lib.load().ccvpe_set_debug(self._handle, int(enable)), "ccvpe_set_debug")

    def read_tap(self, name: str) -> torch.Tensor:
        """Intermediate tensor of the last debug forward as NCHW float32 on the CPU."""
        lib = _lib.load()
        cap = 64 * 1024 * 1024
        while True:
            host = torch.empty(cap, dtype=torch.float32)
            n = C.c_size_t(0)
            shape = (C.c_int32 * 4)()
            rc = lib.ccvpe_read_tap(self._handle, name.encode(), C.c_void_p(host.data_ptr()), cap, C.byref(n), C.byref(shape))
            if rc == -1 and b"needs" in (lib.ccvpe_last_error() or b""):
                cap *= 4
                continue
            _lib.check(rc, f"ccvpe_read_tap({name})")
            return host[: n.value].reshape(*[int(s) for s in shape]).clone()

    def profile(self, grd: torch.Tensor, sat: torch.Tensor):
        """One forward with a hipEvent pair around every launch: list of (name, ms, flops, bytes, issued_flops)."""
        grd, sat = self._prepare(grd, sat)
        B = grd.shape[0]
        lib = _lib.load()
        out, _ = self._alloc_outputs(B, grd.device)
        stream = torch.cuda.current_stream(grd.device).cuda_stream
        n = lib.ccvpe_profile_forward(self._handle, C.c_void_p(grd.data_ptr()), grd.shape[2], grd.shape[3],
                                      C.c_void_p(sat.data_ptr()), B, C.byref(out), C.c_void_p(stream))
        _lib.check(n, "ccvpe_profile_forward")
        self._tuning_sync()
        rows = []
        name = C.create_string_buffer(128)
        ms, fl, by, iss = C.c_float(), C.c_double(), C.c_double(), C.c_double()
        for i in range(n):
            _lib.check(lib.ccvpe_profile_row(self._handle, i, name, 128, C.byref(ms), C.byref(fl), C.byref(by)), "ccvpe_profile_row")
            _lib.check(lib.ccvpe_profile_row_issued(self._handle, i, C.byref(iss)), "ccvpe_profile_row_issued")
            rows.append((name.value.decode(), ms.value, fl.value, by.value, iss.value))
        return rows


class CVM_VIGOR(_CVMBase):
    """models.py:49 - CVM_VIGOR(device, circular_padding)."""
    _variant = "vigor"

    def __init__(self, device, circular_padding, **kw):
        super().__init__(device, circular_padding, None, **kw)


class CVM_VIGOR_ori_prior(_CVMBase):
    """models.py:346 - CVM_VIGOR_ori_prior(device, ori_noise, circular_padding=True)."""
    _variant = "vigor_ori_prior"

    def __init__(self, device, ori_noise, circular_padding=True, **kw):
        super().__init__(device, circular_padding, ori_noise, **kw)


class CVM_KITTI(_CVMBase):
    """models.py:655 - CVM_KITTI(device); no circular padding (models.py:660)."""
    _variant = "kitti"

    def __init__(self, device, **kw):
        super().__init__(device, False, None, **kw)


class CVM_OxfordRobotCar(_CVMBase):
    """models.py:954 - CVM_OxfordRobotCar(device)."""
    _variant = "oxford"

    def __init__(self, device, **kw):
        super().__init__(device, False, None, **kw)
