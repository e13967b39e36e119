"""Stage-by-stage checker of one forward against the oracle, every stage fed the device's own input (teacher forcing).

`check_stages` walks the forward of oracle/ccvpe_oracle.py one stage at a time.  For each stage it
  1. takes the stage's input from the device (`read_tap`, the images, or one of the nine outputs), never from the previous stage of
     the oracle, so errors do not compound and a failure names the launch group that produced it;
  2. computes that one stage with the oracle's functions twice on that input: in fp64 (state dict and input cast up, `ref64`) and
     in fp32 (`ref32`);
  3. records e_ref = max|ref32 - ref64| / max|ref64| - what fp32 arithmetic in another order costs on this very input, the yardstick
     of the tolerance - and e_dev = max|dev - ref64| / max|ref64|, both over the full tensor, with the index of the worst element.

This module imports the oracle and, like the oracle itself, the plain-data tables of `ccvpe_amd.spec` (block schedule, variants, roll
shifts); nothing of the library's code path.  `read_tap` is any callable tap name -> NCHW CPU tensor of the whole
batch (models.read_tap on a debug handle, or a dict of oracle taps in tests/test_stages_cpu.py).

Handed a `PerChannel`, `check_stages` also keeps the same three figures per channel of every 4-D tensor with more than one channel and
position, each relative to the channel's own max |ref64| (`channel_verdict` holds the bounds), and the softmax in the log domain (row
heatmap:log): a tensor whose channel maxima span decades hides its small channels from the full-tensor metric.

Tap layouts the checker relies on (ccvpe_plan.hip):
  - grd_desc{k}: [B, L, 1, 1], the descriptor d[w*c + ch] along dim 1;
  - loc_in{n}:   [B, 8 + C, h, w] = [max score | 7 pad channels | normalize(x)]; the pad channels are not compared;
  - ori_in6:     [B, rpad + D, 8, 8] = [R scores of the full roll set | rpad - R pad channels | normalize(x)], rpad = R rounded up
                 to 8; the pad channels are not compared.
"""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from ccvpe_amd import spec
from oracle import ccvpe_oracle as orc

LOC_IN_PAD = 8          # leading score slot of the loc_in* buffers (1 real channel + 7 pad)


class StageResult(NamedTuple):
    name: str                       # "<stage>" or "<stage>:<tensor>" when a stage writes several tensors
    shape: Tuple[int, ...]
    e_dev: float
    e_ref: float
    worst_index: Tuple[int, ...]    # of |dev - ref64|, in the compared tensor (batch index = position in `samples`)
    launches: Tuple[str, ...]       # prefixes of the plan's launch names that compute this stage (() = no launch of its own)


def launches_of(r: StageResult, launch_names: Sequence[str]) -> List[str]:
    """The launches of a plan (names from its profile rows) that belong to a stage."""
    return [n for n in launch_names if n.startswith(r.launches)]


def _f64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def _unravel(i: int, shape) -> Tuple[int, ...]:
    out = []
    for n in reversed(shape):
        out.append(i % n)
        i //= n
    return tuple(reversed(out))


def _max_err(a: torch.Tensor, ref64: torch.Tensor, weight: Optional[torch.Tensor] = None):
    """max |a - ref64| (* weight) and where."""
    assert a.shape == ref64.shape, (tuple(a.shape), tuple(ref64.shape))
    d = (a.double() - ref64).abs()
    if weight is not None:
        d = d * weight
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)   # a NaN on the device is the worst element
    i = int(d.argmax())
    return d.reshape(-1)[i].item(), _unravel(i, d.shape)


def _result(name, dev, ref32, ref64, launches, weight=None) -> StageResult:
    dev = dev.reshape(ref64.shape)
    scale = max((weight.max() if weight is not None else ref64.abs().max()).item(), 1e-300)
    e_dev, where = _max_err(dev, ref64, weight)
    e_ref, _ = _max_err(ref32, ref64, weight)
    return StageResult(name, tuple(ref64.shape), e_dev / scale, e_ref / scale, where, launches)


class ChannelResult(NamedTuple):
    """The per-channel figures of one compared tensor (channel = dim 1; the maxima run over the checked samples and all positions)."""
    name: str
    shape: Tuple[int, ...]
    scale: torch.Tensor             # [C] s_c = max|ref64_c|
    e_dev: torch.Tensor             # [C] max|dev_c - ref64_c| / s_c; where s_c == 0: 0 if the device is exactly 0 there, else inf
    e_ref: torch.Tensor             # [C] max|ref32_c - ref64_c| / s_c; where s_c == 0: 0
    launches: Tuple[str, ...]


class PerChannel:
    """What check_stages records beside its rows when handed one: a ChannelResult per compared tensor and the row heatmap:log."""

    def __init__(self):
        self.channels: List[ChannelResult] = []
        self.heatmap_log: Optional[StageResult] = None


def _channel_max(t: torch.Tensor) -> torch.Tensor:
    t = torch.where(torch.isnan(t), torch.full_like(t, float("inf")), t)       # a NaN is the worst element
    return t.transpose(0, 1).reshape(t.shape[1], -1).max(dim=1).values


def is_channel_tensor(ref64: torch.Tensor) -> bool:
    """The tensors compared per channel: 4-D, more than one channel, more than one spatial position."""
    return ref64.dim() == 4 and ref64.shape[1] > 1 and ref64.shape[2] * ref64.shape[3] > 1


def _channel_result(name, dev, ref32, ref64, launches) -> ChannelResult:
    dev = dev.reshape(ref64.shape).double()
    s = _channel_max(ref64.abs())
    live = s > 0
    div = torch.where(live, s, torch.ones_like(s))
    e_dev = _channel_max((dev - ref64).abs()) / div
    e_ref = _channel_max((ref32.double() - ref64).abs()) / div
    dead_dev = _channel_max((dev != 0).double()) > 0          # NaN != 0: a NaN in a dead channel fails too
    e_dev = torch.where(live, e_dev, torch.where(dead_dev, torch.full_like(s, float("inf")), torch.zeros_like(s)))
    e_ref = torch.where(live, e_ref, torch.zeros_like(s))
    return ChannelResult(name, tuple(ref64.shape), s, e_dev, e_ref, launches)


FP32_MIN_NORMAL = 2.0 ** -126


def _log_err(p: torch.Tensor, ref64: torch.Tensor):
    """max |log p - log ref64| where ref64 >= 2^-126; below that p may hold 0 or any value <= 2^-126 (anything else, or a NaN: inf)."""
    p = p.double()
    big = ref64 >= FP32_MIN_NORMAL
    d = torch.where(big, (torch.log(p) - torch.log(ref64)).abs(),
                    torch.where((p >= 0) & (p <= FP32_MIN_NORMAL), torch.zeros_like(p), torch.full_like(p, float("inf"))))
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    i = int(d.argmax())
    return d.reshape(-1)[i].item(), _unravel(i, d.shape)


def stem_block0(img, sd, p, circular):
    """Stem (conv + bn0 + swish) and block 0, the first lines of orc.encoder."""
    x = orc._pad_static(img, 3, 2, circular)
    x = orc._swish(orc._bn(F.conv2d(x, sd[p + "._conv_stem.weight"], stride=2), sd, p + "._bn0"))
    return orc.mbconv(x, sd, p + "._blocks.0", spec.B0_BLOCKS[0], circular)


def head_conv(x, sd, p):
    """Head conv + bn1 + swish, the last line of orc.encoder."""
    return orc._swish(orc._bn(F.conv2d(x, sd[p + "._conv_head.weight"]), sd, p + "._bn1"))


def match_cat(score, x):
    """What a matching level hands to its decoder level: cat(max over the rolls, normalize(x)) (orc.forward)."""
    return torch.cat([score.max(dim=1, keepdim=True).values, F.normalize(x, p=2, dim=1)], dim=1)


def check_stages(read_tap: Callable[[str], torch.Tensor], outputs, variant: str, sd, grd: torch.Tensor, sat: torch.Tensor,
                 circular: bool, ori_noise: Optional[float], samples: Optional[Sequence[int]] = None,
                 stages: Optional[Sequence[str]] = None, per_channel: Optional[PerChannel] = None) -> List[StageResult]:
    """Every stage of the forward, see the module docstring.  `outputs`: the nine tensors of the forward (logits, heatmap, ori,
    ms1..ms6) for the whole batch; `grd`, `sat`: the input images of the whole batch; `samples`: batch indices to check (default: all);
    `stages`: prefixes of stage names - only those stages are computed, and only their taps read (default: every stage).
    ("grd_", "match"): the ground encoder, its head and descriptors and the six matching levels, 42 rows; the aerial encoder and the
    decoders are not run, the matching levels still take their x from the device's taps.
    `per_channel`: a PerChannel that receives the per-channel figures of every compared tensor of the computed stages (encoder blocks
    and volumes, sat_descriptor_map, ms* - a channel is a roll -, loc_in* and ori_in6 without their pad channels, the decoder levels)
    and the row heatmap:log; the returned rows are the same with and without it."""
    v = spec.VARIANTS[variant]
    prior = variant == "vigor_ori_prior"
    idx = torch.arange(grd.shape[0]) if samples is None else torch.tensor(list(samples))
    prefixes = None if stages is None else tuple(stages)

    def want(name):
        return prefixes is None or name.startswith(prefixes)
    sd32 = {k: t.detach().cpu() for k, t in sd.items()}
    sd64 = _f64(sd32)
    cache = {}

    def tap(name):                  # the checked samples of a device tap; each tap is read once
        if name not in cache:
            cache[name] = read_tap(name).detach().cpu()[idx].float().clone()
        return cache[name]

    outs = [o.detach()[idx.to(o.device)].cpu().float() for o in outputs]
    out_logits, out_heat, out_ori, out_ms = outs[0], outs[1], outs[2], outs[3:]
    results: List[StageResult] = []

    def stage(name, fn, inputs, dev, launches):
        """fn(sd, *inputs) in fp32 and fp64 against the device tensor(s) `dev` ({suffix: tensor} when the stage writes several)."""
        with torch.no_grad():
            r32 = fn(sd32, *inputs)
            r64 = fn(sd64, *[t.double() for t in inputs])
        if not isinstance(dev, dict):
            dev, r32, r64 = {"": dev}, {"": r32}, {"": r64}
        for key, d in dev.items():
            results.append(_result(name + (":" + key if key else ""), d, r32[key], r64[key], launches))
            if per_channel is not None and is_channel_tensor(r64[key]):
                per_channel.channels.append(_channel_result(results[-1].name, d, r32[key], r64[key], launches))

    # ---- encoders ----
    for tag, img, circ in (("grd", grd[idx].float(), circular), ("sat", sat[idx].float(), False)):
        p = tag + "_efficientnet"
        if want(f"{tag}_block0"):
            stage(f"{tag}_block0", lambda s, x: stem_block0(x, s, p, circ), [img], tap(f"{tag}_block0"), (f"{tag}.stem", f"{tag}.b0."))
        for i in range(1, len(spec.B0_BLOCKS)):
            if want(f"{tag}_block{i}"):
                stage(f"{tag}_block{i}", lambda s, x: orc.mbconv(x, s, f"{p}._blocks.{i}", spec.B0_BLOCKS[i], circ),
                      [tap(f"{tag}_block{i - 1}")], tap(f"{tag}_block{i}"), (f"{tag}.b{i}.",))
        if want(f"{tag}_volume"):
            stage(f"{tag}_volume", lambda s, x: head_conv(x, s, p), [tap(f"{tag}_block15")], tap(f"{tag}_volume"), (f"{tag}.head",))

    # ---- descriptors ----
    for k in range(1, 7):
        if want(f"grd_desc{k}"):
            stage(f"grd_desc{k}", lambda s, x: orc.ground_descriptor(x, s, k), [tap("grd_volume")],
                  tap(f"grd_desc{k}").flatten(1), ("grd.heads", "grd.desc"))
    if want("sat_descriptor_map"):
        stage("sat_descriptor_map", lambda s, x: orc.aerial_descriptor_map(x, s), [tap("sat_volume")], tap("sat_descriptor_map"),
              ("sat.descmap",))

    # ---- matching levels: x and the ground descriptor -> ms{k}, the maximum over the rolls, loc_in{7-k} (and ori_in6 at level 1) ----
    def real_loc_in(n):
        t = tap(f"loc_in{n}")
        return torch.cat([t[:, :1], t[:, LOC_IN_PAD:]], dim=1)

    n_rolls = v.n_rolls
    D = v.match_ch[0]

    def real_ori_in6():
        t = tap("ori_in6")
        rpad = t.shape[1] - D
        assert rpad >= n_rolls
        return torch.cat([t[:, :n_rolls], t[:, rpad:]], dim=1)

    for k in range(1, 7):
        n = 7 - k
        level = f"loc_level{n}" if n >= 2 else "logits"
        if not (want(f"match{k}") or want(level)):
            continue
        x = tap("sat_descriptor_map") if k == 1 else tap(f"loc_level{8 - k}")
        g = tap(f"grd_desc{k}").flatten(1)
        L = g.shape[1]
        shifts = spec.roll_shifts(v, k, L, ori_noise)
        full = spec.full_roll_shifts(v, 1, L) if k == 1 else None

        def match(s, x, g):
            score = orc.rolling_match(x, g, shifts)
            # the maximum also as a row of its own: inside loc_in{n} it is scaled by the normalised features (up to 1 against scores of 0.1-0.2)
            out = {"ms": score, "max": score.max(dim=1, keepdim=True).values, f"loc_in{n}": match_cat(score, x)}
            if k == 1:   # the full roll set: returned as ms1 and fed to the orientation decoder (the restricted set's maximum enters loc_in6)
                out["ms"] = orc.rolling_match(x, g, full) if prior else score
                out["ori_in6"] = torch.cat([out["ms"], F.normalize(x, p=2, dim=1)], dim=1)
            return out

        if want(f"match{k}"):
            dev = {"ms": out_ms[k - 1], "max": tap(f"loc_in{n}")[:, :1], f"loc_in{n}": real_loc_in(n)}
            if k == 1:
                dev["ori_in6"] = real_ori_in6()
            stage(f"match{k}", match, [x, g], dev, (f"match{k}",))

        # ---- localisation decoder level n ----
        if not want(level):
            continue
        if n >= 2:
            skip = tap(f"sat_block{spec.TAP_BLOCKS[k - 1]}")
            stage(f"loc_level{n}", lambda s, x, sk: orc._decoder_level(x, sk, s, n, ""), [real_loc_in(n), skip], tap(f"loc_level{n}"),
                  (f"loc{n}.",))
        else:
            stage("logits", lambda s, x: orc._decoder_level(x, None, s, 1, ""), [real_loc_in(1)], out_logits, ("loc1.",))

    # ---- softmax ----
    def softmax(s, lg):
        heat = torch.softmax(lg.flatten(1), dim=-1)
        return {"": heat, "over_max": heat / heat.max(dim=1, keepdim=True).values}

    hd = out_heat.flatten(1)
    if want("heatmap"):
        stage("heatmap", softmax, [out_logits], {"": hd, "over_max": hd / hd.max(dim=1, keepdim=True).values}, ("softmax",))
        if per_channel is not None:     # the tail of a peaked softmax is invisible next to its maximum: the same stage in the log domain
            with torch.no_grad():
                h64 = softmax(None, out_logits.double())[""]
                e_dev, where = _log_err(hd, h64)
                e_ref, _ = _log_err(softmax(None, out_logits)[""], h64)
            per_channel.heatmap_log = StageResult("heatmap:log", tuple(h64.shape), e_dev, e_ref, where, ("softmax",))

    # ---- orientation decoder ----
    for n in range(6, 1, -1):
        if not want(f"ori_level{n}"):
            continue
        xo = real_ori_in6() if n == 6 else tap(f"ori_level{n + 1}")
        skip = tap(f"sat_block{spec.TAP_BLOCKS[6 - n]}")
        stage(f"ori_level{n}", lambda s, x, sk: orc._decoder_level(x, sk, s, n, "_ori"), [xo, skip], tap(f"ori_level{n}"), (f"ori{n}.",))
    if want("ori_level1"):
        stage("ori_level1", lambda s, x: orc._decoder_level(x, None, s, 1, "_ori"), [tap("ori_level2")], tap("ori_level1_nchw"), ("ori1.",))

    # ---- normalise: weighted by the magnitude of the un-normalised vector (tests/test_parity_gpu.py ori_weighted_error) ----
    if not want("ori"):
        return results
    raw = tap("ori_level1_nchw")
    mag = raw.double().pow(2).sum(dim=1, keepdim=True).sqrt()
    with torch.no_grad():
        results.append(_result("ori", out_ori, F.normalize(raw, p=2, dim=1), F.normalize(raw.double(), p=2, dim=1), ("ori1.",), weight=mag))
    return results


# Tolerances.  The yardstick is e_ref, measured on the stage's own input by the reference arithmetic, never by the code under test.
BOUND_FP32 = 2e-5       # what tests/test_ops_gpu.py holds the implicit-GEMM and F(2x2) tiles to
BOUND_F4 = 1e-4         # ... and the F(4x4) Winograd tiles and every bf16x3 tile to
REF_FACTOR = 8.0        # another summation order over K up to 11520, hardware exp and reciprocal


def bound(r: StageResult, f4: bool = False, bf16x3: bool = False, factor: float = REF_FACTOR) -> float:
    """The largest e_dev a stage may show: min(2e-5, factor * e_ref), or 1e-4 where one of its launches ran an F(4x4) Winograd tile
    or the handle runs in bf16x3 precision."""
    if f4 or bf16x3:
        return BOUND_F4
    return min(BOUND_FP32, factor * r.e_ref)


class ChannelVerdict(NamedTuple):
    name: str
    n_channels: int
    worst: int                      # the asserted channel with the largest e_dev / bound
    e_dev: float                    # ... its figures
    e_ref: float
    scale: float
    bound: float
    over: Tuple[int, ...]           # asserted channels over their bound (dead channels the device did not leave exactly 0 included)
    excluded: Tuple[int, ...]       # ill-conditioned channels, left out of the assertion

    @property
    def ok(self) -> bool:
        return not self.over and len(self.excluded) <= MAX_EXCLUDED * self.n_channels


MAX_EXCLUDED = 0.01     # of a stage's channels


BF16X3_OPERAND = 2.0 ** 7   # a bf16x3 operand hi + lo keeps 16 significand bits: 2^-17 against the 2^-24 of an fp32 rounding


def channel_verdict(c: ChannelResult, f4: bool = False, bf16x3: bool = False, factor: float = REF_FACTOR) -> ChannelVerdict:
    """Every channel of a compared tensor against its own bound, relative to its own scale s_c.  The yardstick of a channel is
    y_c = max(e_ref_c, median of e_ref over the tensor's live channels) - the reference's own error on the device's own input; the
    median floor covers a channel where the fp32 and the fp64 oracle happen to agree (a constant channel swish(bias)).
      - factor * y_c;
      - BOUND_F4 where the stage ran an F(4x4) Winograd tile;
      - max(BOUND_F4, BF16X3_OPERAND * y_c) on a bf16x3 handle.  Flat BOUND_F4 is out of reach of the format on a channel that
        cancels: the error of a bf16x3 dot product is 2^-17 of its operands where fp32's is 2^-24, so both grow with the channel's
        conditioning, which e_ref_c measures.  Exact sums of the three bf16 products of the aerial descriptor map reach 1.6e-4 of a
        channel's maximum and 61 * y_c on the Oxford batch-3 stress case (tests/test_stages_cpu.py asserts both sides, no GPU);
      - exactly 0 where s_c == 0.
    A channel with REF_FACTOR * e_ref_c > BOUND_F4 is ill-conditioned on this input and left out; at most MAX_EXCLUDED of the channels."""
    live = c.scale > 0
    median = c.e_ref[live].median().item() if live.any() else 0.0
    yardstick = c.e_ref.clamp(min=median)
    b = factor * yardstick
    if bf16x3:
        b = (BF16X3_OPERAND * yardstick).clamp(min=BOUND_F4)
    elif f4:
        b = torch.full_like(b, BOUND_F4)
    b = torch.where(live, b, torch.zeros_like(b))
    excluded = live & (REF_FACTOR * c.e_ref > BOUND_F4)
    over = ~excluded & ~(c.e_dev <= b)
    ratio = torch.where(excluded, torch.full_like(b, -1.0), torch.where(b > 0, c.e_dev / b.clamp(min=1e-300), c.e_dev))
    w = int(ratio.argmax())
    return ChannelVerdict(c.name, len(b), w, c.e_dev[w].item(), c.e_ref[w].item(), c.scale[w].item(), b[w].item(),
                          tuple(over.nonzero().flatten().tolist()), tuple(excluded.nonzero().flatten().tolist()))


def heatmap_log_bound(r: StageResult, factor: float = REF_FACTOR) -> float:
    """The largest |log dev - log ref64| of the row heatmap:log: factor * the fp32 oracle's own."""
    return factor * r.e_ref


def format_channel_table(channels: Sequence[ChannelResult], verdicts: Sequence[ChannelVerdict]) -> str:
    rows = [f"{'stage':24s} {'C':>5s} {'s_min':>9s} {'s_max':>9s} {'e_ref med':>9s} {'e_ref max':>9s} | worst channel: "
            f"{'c':>5s} {'s_c':>9s} {'e_dev_c':>9s} {'e_ref_c':>9s} {'bound_c':>9s} {'over':>5s} {'excl':>5s}"]
    for c, v in zip(channels, verdicts):
        live = c.scale > 0
        s_min = c.scale[live].min().item() if live.any() else 0.0
        med = c.e_ref[live].median().item() if live.any() else 0.0
        rows.append(f"{c.name:24s} {v.n_channels:5d} {s_min:9.2e} {c.scale.max().item():9.2e} {med:9.2e} {c.e_ref.max().item():9.2e} | "
                    f"               {v.worst:5d} {v.scale:9.2e} {v.e_dev:9.2e} {v.e_ref:9.2e} {v.bound:9.2e} {len(v.over):5d} {len(v.excluded):5d}")
    return "\n".join(rows)


def format_table(results: Sequence[StageResult]) -> str:
    rows = [f"{'stage':24s} {'shape':22s} {'e_dev':>9s} {'e_ref':>9s}  worst"]
    for r in results:
        rows.append(f"{r.name:24s} {'x'.join(map(str, r.shape)):22s} {r.e_dev:9.2e} {r.e_ref:9.2e}  {r.worst_index}")
    return "\n".join(rows)
