"""The Python front end without a GPU: which of two simultaneous faults a method reports - the order of its check
groups, recorded from the methods as they stood before they shared one call skeleton -, that what the forms share is written once,
and that every public method kept its signature and docstring."""
import hashlib
import inspect
import re

import numpy as np
import pytest
import torch

from ccvpe_amd import aerial, models

N = 512 * 512
_M = {}


def model(training=False):
    if training not in _M:
        m = models.CVM_OxfordRobotCar("cpu")
        _M[training] = m.train() if training else m.eval()
    return _M[training]


# ---- inputs: every tensor is on the host, so a call that is valid up to its device check ends there -------------------------------
G, S = torch.zeros(2, 3, 154, 231), torch.zeros(2, 3, 512, 512)
G_BAD, S_BAD = torch.zeros(2, 4, 154, 231), torch.zeros(2, 3, 512, 511)
CACHE = torch.zeros(16)
LG, ORI = torch.zeros(2, N), torch.zeros(2, 2, 512, 512)
LG_BAD = torch.zeros(2, N - 1)
LP = torch.zeros(512, 512)                       # well formed, but on the host
LP_SHAPE = torch.zeros(3, 512, 512)              # one map too many for B = 2
LP_F64 = torch.zeros(512, 512, dtype=torch.float64)
LP_STRIDED = torch.zeros(512, 1024)[:, ::2]
TB, TB_BAD = torch.zeros(73), torch.zeros(3, 73)
IDX_BAD = [0, 1, 1]
BEL, BEL_BAD = torch.zeros(2, 512, 512), torch.zeros(2, 512, 511)
HIST, HIST_BAD = torch.zeros(2, 72), torch.zeros(72)
TAPS, TAPS_BAD, TAPS_LONG = np.ones(4, np.float32), np.ones((3, 4), np.float32), np.ones(34, np.float32)
MAT, MAT_BAD = np.array([1.0, 0, 0, 0, 1, 0]), np.zeros((3, 6))
SHIFT, SHIFT_BAD = np.zeros((2, 2)), np.zeros((3, 2))
LEVELS, LEVELS_BAD = (0.5, 0.9), (0.5, 1.5)
TILES, TILES_BAD = [[0], [1]], [[0], []]

EVAL, EVAL_LONG = r"call \.eval\(\) first$", r"call \.eval\(\) first \(reference test loops do"
NO_CPU = r"no CPU path: inputs must live"
NO_CPU_HELD = r"no CPU path: logits and ori must live"
GRD_CUDA = r"grd must be a cuda tensor \[B,3,H,W\]"
LP_CUDA = r"log_prior must be a cuda tensor on the inputs' device, not a cpu tensor"
LP_FORM = r"log_prior must be \[512,512\], \[1,512,512\], \[2,512,512\] or"
TB_FORM = r"heading_log_prior must be \[nb\+1\] or \[2, nb\+1\]"
TB_CUDA = r"heading_log_prior must be a cuda tensor on the inputs' device"
IDX = r"tile_index must hold one tile per query"
HELD = r"expected logits \[B,512\*512\] and ori \[B,2,512,512\]"
RADIUS, BINS, LEV = r"radius must be in 0\.\.32", r"bins must be in 4\.\.360", r"every level must be finite and in \(0, 1\]"
MAPS = r"belief must be \[B,512,512\] or \[B,1,512,512\], got \(2, 512, 511\)"
BEL_CUDA = r"belief must be a cuda tensor, not a cpu tensor"
TAPS_FORM = r"taps must be \[radius\+1\] or \[2, radius\+1\], got \(3, 4\)"
FLOOR = r"floor must be >= 0"
R, V = RuntimeError, ValueError

# (id, training, call, exception, message): every call carries two faults, one of each of two neighbouring check groups - training
# mode (T), the method's own arguments (A), the input shape (S), the input's device (D), the prior (P), the tile_index form (I) - or is
# valid up to its device check ("ends")
CASES = [
    # the plain forms: the image side checks device before shape; the cached side the index, then grd
    ("localize T>D", 1, lambda m: m.localize(G, S), R, EVAL_LONG),
    ("localize D>S", 0, lambda m: m.localize(G, S_BAD), R, NO_CPU),
    ("forward T>D", 1, lambda m: m(G, S), R, EVAL_LONG),
    ("forward D>S", 0, lambda m: m(G_BAD, S), R, NO_CPU),
    ("localize_cached T>I", 1, lambda m: m.localize_cached(G, CACHE, IDX_BAD), R, EVAL),
    ("localize_cached I>S", 0, lambda m: m.localize_cached(G_BAD, CACHE, IDX_BAD), V, IDX),
    ("localize_cached ends", 0, lambda m: m.localize_cached(G, CACHE), V, GRD_CUDA),
    ("forward_cached T>I", 1, lambda m: m.forward_cached(G, CACHE, IDX_BAD), R, EVAL),
    ("forward_cached I>S", 0, lambda m: m.forward_cached(G_BAD, CACHE, IDX_BAD), V, IDX),
    # top-K: its own arguments after the inputs on every side
    ("localize_topk T>A", 1, lambda m: m.localize_topk(G, S, 0, 0), R, EVAL_LONG),
    ("localize_topk D>A", 0, lambda m: m.localize_topk(G, S, 0, 0), R, NO_CPU),
    ("localize_topk_cached T>I", 1, lambda m: m.localize_topk_cached(G, CACHE, 0, 0, IDX_BAD), R, EVAL),
    ("localize_topk_cached I>S", 0, lambda m: m.localize_topk_cached(G_BAD, CACHE, 0, 0, IDX_BAD), V, IDX),
    ("localize_topk_cached S>A", 0, lambda m: m.localize_topk_cached(G, CACHE, 0, 0), V, GRD_CUDA),
    ("postprocess_topk T>D", 1, lambda m: m.postprocess_topk(BEL, ORI, 0, 0), R, EVAL),
    ("postprocess_topk D>A", 0, lambda m: m.postprocess_topk(BEL, ORI, 0, 0), R, r"no CPU path: heatmap and ori"),
    # position prior
    ("localize_prior T>A", 1, lambda m: m.localize_prior(G, S, LP, k=65), R, EVAL),
    ("localize_prior A>P", 0, lambda m: m.localize_prior(G, S, LP_SHAPE, k=65), V, r"k must be in 0\.\.64"),
    ("localize_prior A(radius)>P", 0, lambda m: m.localize_prior(G, S, LP_SHAPE, k=0, radius=3), V, r"radius 3 needs k >= 1"),
    ("localize_prior P>S", 0, lambda m: m.localize_prior(G, S_BAD, LP_SHAPE), V, LP_FORM),
    ("localize_prior P(dtype)>D", 0, lambda m: m.localize_prior(G, S, LP_F64), V, r"log_prior must be float32"),
    ("localize_prior P(contiguous)>D", 0, lambda m: m.localize_prior(G, S, LP_STRIDED), V, r"log_prior must be contiguous"),
    ("localize_prior P(device)>D", 0, lambda m: m.localize_prior(G, S_BAD, LP), V, LP_CUDA),
    ("localize_prior_cached T>I", 1, lambda m: m.localize_prior_cached(G, CACHE, LP_SHAPE, tile_index=IDX_BAD), R, EVAL),
    ("localize_prior_cached I>S", 0, lambda m: m.localize_prior_cached(G_BAD, CACHE, LP, tile_index=IDX_BAD), V, IDX),
    ("localize_prior_cached S>A", 0, lambda m: m.localize_prior_cached(G, CACHE, LP_SHAPE, k=65), V, GRD_CUDA),
    ("postprocess_prior T>S", 1, lambda m: m.postprocess_prior(LG_BAD, ORI, LP), R, EVAL),
    ("postprocess_prior S>A", 0, lambda m: m.postprocess_prior(LG_BAD, ORI, LP, k=65), V, HELD),
    ("postprocess_prior A>P", 0, lambda m: m.postprocess_prior(LG, ORI, LP_SHAPE, k=65), V, r"k must be in 0\.\.64"),
    ("postprocess_prior P>D", 0, lambda m: m.postprocess_prior(LG, ORI, LP_SHAPE), V, LP_FORM),
    ("postprocess_prior P(device)>D", 0, lambda m: m.postprocess_prior(LG, ORI, LP), V, LP_CUDA),
    # track update
    ("track_update T>P", 1, lambda m: m.track_update(G, S, LP_SHAPE), R, EVAL),
    ("track_update P>S", 0, lambda m: m.track_update(G, S_BAD, LP_SHAPE), V, LP_FORM),
    ("track_update P(device)>D", 0, lambda m: m.track_update(G, S, LP), V, LP_CUDA),
    ("track_update ends", 0, lambda m: m.track_update(G, S), R, NO_CPU),
    ("track_update D>S", 0, lambda m: m.track_update(G, S_BAD), R, NO_CPU),
    ("track_update_cached T>I", 1, lambda m: m.track_update_cached(G, CACHE, LP_SHAPE, tile_index=IDX_BAD), R, EVAL),
    ("track_update_cached I>S", 0, lambda m: m.track_update_cached(G_BAD, CACHE, None, tile_index=IDX_BAD), V, IDX),
    ("track_update_cached S>P", 0, lambda m: m.track_update_cached(G, CACHE, LP_SHAPE), V, GRD_CUDA),
    ("track_update_logits T>S", 1, lambda m: m.track_update_logits(LG_BAD, ORI), R, EVAL),
    ("track_update_logits S>P", 0, lambda m: m.track_update_logits(LG_BAD, ORI, LP_SHAPE), V, HELD),
    ("track_update_logits P>D", 0, lambda m: m.track_update_logits(LG, ORI, LP_SHAPE), V, LP_FORM),
    ("track_update_logits ends", 0, lambda m: m.track_update_logits(LG, ORI), R, NO_CPU_HELD),
    # summary
    ("localize_summary T>A", 1, lambda m: m.localize_summary(G, S, radius=33), R, EVAL),
    ("localize_summary A>P", 0, lambda m: m.localize_summary(G, S, LP_SHAPE, radius=33), V, RADIUS),
    ("localize_summary P>S", 0, lambda m: m.localize_summary(G, S_BAD, LP_SHAPE), V, LP_FORM),
    ("localize_summary A>D", 0, lambda m: m.localize_summary(G, S, radius=-1), V, RADIUS),
    ("localize_summary ends", 0, lambda m: m.localize_summary(G, S), R, NO_CPU),
    ("localize_summary_cached T>I", 1, lambda m: m.localize_summary_cached(G, CACHE, radius=33, tile_index=IDX_BAD), R, EVAL),
    ("localize_summary_cached I>S", 0, lambda m: m.localize_summary_cached(G_BAD, CACHE, tile_index=IDX_BAD), V, IDX),
    ("localize_summary_cached S>A", 0, lambda m: m.localize_summary_cached(G, CACHE, radius=33), V, GRD_CUDA),
    ("postprocess_summary T>S", 1, lambda m: m.postprocess_summary(LG_BAD, ORI), R, EVAL),
    ("postprocess_summary S>A", 0, lambda m: m.postprocess_summary(LG_BAD, ORI, radius=33), V, HELD),
    ("postprocess_summary A>P", 0, lambda m: m.postprocess_summary(LG, ORI, LP_SHAPE, radius=33), V, RADIUS),
    ("postprocess_summary P>D", 0, lambda m: m.postprocess_summary(LG, ORI, LP_SHAPE), V, LP_FORM),
    ("postprocess_summary ends", 0, lambda m: m.postprocess_summary(LG, ORI, posterior=True), R, NO_CPU_HELD),
    # heading: the cached and the held side check bins and radius before anything else, the image side after training mode
    ("localize_heading T>A", 1, lambda m: m.localize_heading(G, S, bins=3), R, EVAL),
    ("localize_heading A(bins)>A(radius)", 0, lambda m: m.localize_heading(G, S, radius=33, bins=3), V, BINS),
    ("localize_heading A>P", 0, lambda m: m.localize_heading(G, S, LP_SHAPE, radius=33), V, RADIUS),
    ("localize_heading P>S", 0, lambda m: m.localize_heading(G, S_BAD, LP_SHAPE), V, LP_FORM),
    ("localize_heading ends", 0, lambda m: m.localize_heading(G, S, summary=True), R, NO_CPU),
    ("localize_heading_cached A(bins)>T", 1, lambda m: m.localize_heading_cached(G, CACHE, bins=3, tile_index=IDX_BAD), V, BINS),
    ("localize_heading_cached A(radius)>T", 1, lambda m: m.localize_heading_cached(G, CACHE, radius=33), V, RADIUS),
    ("localize_heading_cached T>I", 1, lambda m: m.localize_heading_cached(G, CACHE, tile_index=IDX_BAD), R, EVAL),
    ("localize_heading_cached I>S", 0, lambda m: m.localize_heading_cached(G_BAD, CACHE, tile_index=IDX_BAD), V, IDX),
    ("localize_heading_cached A>S", 0, lambda m: m.localize_heading_cached(G, CACHE, radius=33, bins=3), V, BINS),
    ("localize_heading_cached S>P", 0, lambda m: m.localize_heading_cached(G, CACHE, LP_SHAPE), V, GRD_CUDA),
    ("postprocess_heading T>S", 1, lambda m: m.postprocess_heading(LG_BAD, ORI), R, EVAL),
    ("postprocess_heading A>T", 1, lambda m: m.postprocess_heading(LG_BAD, ORI, bins=3), V, BINS),
    ("postprocess_heading A>S", 0, lambda m: m.postprocess_heading(LG_BAD, ORI, radius=33), V, RADIUS),
    ("postprocess_heading S>P", 0, lambda m: m.postprocess_heading(LG_BAD, ORI, LP_SHAPE), V, HELD),
    ("postprocess_heading A>P", 0, lambda m: m.postprocess_heading(LG, ORI, LP_SHAPE, bins=361), V, BINS),
    ("postprocess_heading P>D", 0, lambda m: m.postprocess_heading(LG, ORI, LP_SHAPE), V, LP_FORM),
    ("postprocess_heading ends", 0, lambda m: m.postprocess_heading(LG, ORI), R, NO_CPU_HELD),
    # heading prior: the cached form, too, checks its own arguments first
    ("localize_heading_prior T>A", 1, lambda m: m.localize_heading_prior(G, S, TB_BAD, bins=3), R, EVAL),
    ("localize_heading_prior A>P", 0, lambda m: m.localize_heading_prior(G, S, TB_BAD, LP_SHAPE, bins=3), V, BINS),
    ("localize_heading_prior P>P(table)", 0, lambda m: m.localize_heading_prior(G, S, TB_BAD, LP_SHAPE), V, LP_FORM),
    ("localize_heading_prior P(table)>S", 0, lambda m: m.localize_heading_prior(G, S_BAD, TB_BAD), V, TB_FORM),
    ("localize_heading_prior P(device)>D", 0, lambda m: m.localize_heading_prior(G, S, TB), V, TB_CUDA),
    ("localize_heading_prior_cached T>A", 1, lambda m: m.localize_heading_prior_cached(G, CACHE, TB_BAD, bins=3), R, EVAL),
    ("localize_heading_prior_cached A>I", 0, lambda m: m.localize_heading_prior_cached(G, CACHE, TB, bins=3, tile_index=IDX_BAD), V, BINS),
    ("localize_heading_prior_cached P(table)>I", 0, lambda m: m.localize_heading_prior_cached(G, CACHE, TB_BAD, tile_index=IDX_BAD), V, TB_FORM),
    ("localize_heading_prior_cached P(device)>S", 0, lambda m: m.localize_heading_prior_cached(G_BAD, CACHE, TB), V, TB_CUDA),
    ("heading_prior_map T>S", 1, lambda m: m.heading_prior_map(BEL, TB), R, EVAL),
    ("heading_prior_map S>P", 0, lambda m: m.heading_prior_map(BEL, TB_BAD, LP_SHAPE), V, r"ori must be \[B,2,512,512\]"),
    ("heading_prior_map P>P(table)", 0, lambda m: m.heading_prior_map(ORI, TB_BAD, LP_SHAPE), V, LP_FORM),
    ("heading_prior_map P(table)>D", 0, lambda m: m.heading_prior_map(ORI, TB_BAD), V, TB_FORM),
    ("heading_prior_map P(device)>D", 0, lambda m: m.heading_prior_map(ORI, TB), V, TB_CUDA),
    # credible: the image side checks training first, the other two the levels
    ("localize_credible T>A", 1, lambda m: m.localize_credible(G, S, LEVELS_BAD), R, EVAL),
    ("localize_credible A>P", 0, lambda m: m.localize_credible(G, S, LEVELS_BAD, LP_SHAPE), V, LEV),
    ("localize_credible P>A(probe)", 0, lambda m: m.localize_credible(G, S, LEVELS, LP_SHAPE, probe=[0.5, 1.0]), V, LP_FORM),
    ("localize_credible A(probe)>S", 0, lambda m: m.localize_credible(G, S_BAD, LEVELS, probe=[1, 2, 3]), V, r"probe must hold one integer"),
    ("localize_credible ends", 0, lambda m: m.localize_credible(G, S, LEVELS, probe=[1, 2], level_map=True), R, NO_CPU),
    ("localize_credible_cached A>T", 1, lambda m: m.localize_credible_cached(G, CACHE, LEVELS_BAD), V, LEV),
    ("localize_credible_cached T>I", 1, lambda m: m.localize_credible_cached(G, CACHE, LEVELS, tile_index=IDX_BAD), R, EVAL),
    ("localize_credible_cached I>S", 0, lambda m: m.localize_credible_cached(G_BAD, CACHE, LEVELS, tile_index=IDX_BAD), V, IDX),
    ("localize_credible_cached S>P", 0, lambda m: m.localize_credible_cached(G, CACHE, LEVELS, LP_SHAPE), V, GRD_CUDA),
    ("postprocess_credible A>T", 1, lambda m: m.postprocess_credible(LG, ORI, LEVELS_BAD), V, LEV),
    ("postprocess_credible T>S", 1, lambda m: m.postprocess_credible(LG_BAD, ORI, LEVELS), R, EVAL),
    ("postprocess_credible S>P", 0, lambda m: m.postprocess_credible(LG_BAD, ORI, LEVELS, LP_SHAPE), V, HELD),
    ("postprocess_credible P>A(probe)", 0, lambda m: m.postprocess_credible(LG, ORI, LEVELS, LP_SHAPE, probe=[1, 2, 3]), V, LP_FORM),
    ("postprocess_credible A(probe)>D", 0, lambda m: m.postprocess_credible(LG, ORI, LEVELS, probe=[1, 2, 3]), V, r"probe must hold one integer"),
    ("postprocess_credible ends", 0, lambda m: m.postprocess_credible(LG, ORI, LEVELS, probe=[1, 2]), R, NO_CPU_HELD),
    # the stored-map methods
    ("belief_summary T>S", 1, lambda m: m.belief_summary(BEL_BAD), R, EVAL),
    ("belief_summary S>A", 0, lambda m: m.belief_summary(BEL_BAD, radius=33), V, MAPS),
    ("belief_summary S(type)", 0, lambda m: m.belief_summary(BEL.numpy(), radius=33), V, r"belief must be a float32 cuda tensor \[B,512,512\]"),
    ("belief_summary S(dtype)>A", 0, lambda m: m.belief_summary(BEL.double(), radius=33), V, r"belief must be float32, got torch.float64"),
    ("belief_summary S(contiguous)>A", 0, lambda m: m.belief_summary(torch.zeros(2, 512, 1024)[:, :, ::2], radius=33), V, r"belief must be contiguous"),
    ("belief_summary A>D", 0, lambda m: m.belief_summary(BEL, radius=33), V, RADIUS),
    ("belief_summary ends", 0, lambda m: m.belief_summary(BEL.view(2, 1, 512, 512)), V, BEL_CUDA),
    ("belief_credible T>S", 1, lambda m: m.belief_credible(BEL_BAD, LEVELS), R, EVAL),
    ("belief_credible S>A", 0, lambda m: m.belief_credible(BEL_BAD, LEVELS_BAD), V, MAPS),
    ("belief_credible A>D", 0, lambda m: m.belief_credible(BEL, LEVELS_BAD), V, LEV),
    ("belief_credible D>A(probe)", 0, lambda m: m.belief_credible(BEL, LEVELS, probe=[1, 2, 3]), V, BEL_CUDA),
    # the predict methods
    ("track_predict T>S", 1, lambda m: m.track_predict(BEL_BAD, SHIFT, TAPS, 0.0), R, EVAL),
    ("track_predict S>taps", 0, lambda m: m.track_predict(BEL_BAD, SHIFT, TAPS_BAD, 0.0), V, MAPS),
    ("track_predict taps>floor", 0, lambda m: m.track_predict(BEL, SHIFT, TAPS_BAD, -1.0), V, TAPS_FORM),
    ("track_predict radius>floor", 0, lambda m: m.track_predict(BEL, SHIFT, TAPS_LONG, -1.0), V, r"taps give radius 33, must be in 0\.\.32$"),
    ("track_predict floor>shift", 0, lambda m: m.track_predict(BEL, SHIFT_BAD, TAPS, -1.0), V, FLOOR),
    ("track_predict shift>D", 0, lambda m: m.track_predict(BEL, SHIFT_BAD, TAPS, 0.0), V, r"shift_px must have shape \(2, 2\), got \(3, 2\)"),
    ("track_predict ends", 0, lambda m: m.track_predict(BEL, SHIFT, TAPS, 0.0), V, BEL_CUDA),
    ("track_predict_affine T>S", 1, lambda m: m.track_predict_affine(BEL_BAD, MAT, TAPS, 0.0), R, EVAL),
    ("track_predict_affine S>matrix", 0, lambda m: m.track_predict_affine(BEL_BAD, MAT_BAD, TAPS, 0.0), V, MAPS),
    ("track_predict_affine matrix>taps", 0, lambda m: m.track_predict_affine(BEL, MAT_BAD, TAPS_BAD, 0.0), V, r"matrix must be \[6\] or \[2, 6\]"),
    ("track_predict_affine taps>floor", 0, lambda m: m.track_predict_affine(BEL, MAT, TAPS_BAD, -1.0), V, TAPS_FORM),
    ("track_predict_affine radius>floor", 0, lambda m: m.track_predict_affine(BEL, MAT, TAPS_LONG, -1.0), V, r"taps give radius 33, must be in 0\.\.32$"),
    ("track_predict_affine floor>D", 0, lambda m: m.track_predict_affine(BEL, MAT, TAPS, -1.0), V, FLOOR),
    ("track_predict_affine ends", 0, lambda m: m.track_predict_affine(BEL, MAT, TAPS, 0.0), V, BEL_CUDA),
    ("heading_predict T>S", 1, lambda m: m.heading_predict(HIST_BAD, 0.0, TAPS, 0.0), R, EVAL),
    ("heading_predict S>taps", 0, lambda m: m.heading_predict(HIST_BAD, 0.0, TAPS_BAD, 0.0), V, r"hist must be a float32 cuda tensor \[B, nb\]"),
    ("heading_predict taps>floor", 0, lambda m: m.heading_predict(HIST, 0.0, TAPS_BAD, -1.0), V, TAPS_FORM),
    ("heading_predict radius>floor", 0, lambda m: m.heading_predict(torch.zeros(2, 6), 0.0, TAPS, -1.0), V,
     r"taps give radius 3, must be in 0\.\.32 with 2 radius \+ 1 <= nb = 6"),
    ("heading_predict floor>turn", 0, lambda m: m.heading_predict(HIST, [0.0, 1.0, 2.0], TAPS, -1.0), V, FLOOR),
    ("heading_predict turn>D", 0, lambda m: m.heading_predict(HIST, [0.0, 1.0, 2.0], TAPS, 0.0), V, r"turn_deg must have shape \(2,\)"),
    ("heading_predict ends", 0, lambda m: m.heading_predict(HIST, 0.0, TAPS, 0.0), V, r"hist must be a cuda tensor, not a cpu tensor"),
    # the encoders and the region forms
    ("encode_aerial T>S", 1, lambda m: m.encode_aerial(S_BAD), R, EVAL),
    ("encode_aerial ends", 0, lambda m: m.encode_aerial(S), V, r"sat must be a cuda tensor \[B,3,512,512\]"),
    ("encode_ground T>S", 1, lambda m: m.encode_ground(G_BAD), R, EVAL),
    ("encode_ground ends", 0, lambda m: m.encode_ground(G), V, GRD_CUDA),
    ("localize_region T>A", 1, lambda m: m.localize_region(CACHE, CACHE, TILES_BAD), R, EVAL),
    ("localize_region A>D", 0, lambda m: m.localize_region(CACHE, CACHE, TILES_BAD), V, r"tiles\[1\] is empty"),
    ("localize_region ends", 0, lambda m: m.localize_region(CACHE, CACHE, TILES), V, r"ground_cache must be the cuda tensor encode_ground returned"),
    ("localize_region_prior A>P", 0, lambda m: m.localize_region_prior(CACHE, CACHE, TILES_BAD, LP_SHAPE), V, r"tiles\[1\] is empty"),
    ("localize_region_prior P>D", 0, lambda m: m.localize_region_prior(CACHE, CACHE, TILES, LP_SHAPE), V, LP_FORM),
    ("localize_region_prior P(None)>D", 0, lambda m: m.localize_region_prior(CACHE, CACHE, TILES, None), V, r"log_prior must be a float32 cuda tensor"),
]


def test_case_ids_are_unique():
    ids = [c[0] for c in CASES]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_error_precedence(case):
    _, training, call, exc, message = case
    with pytest.raises(exc, match=message) as info:
        call(model(bool(training)))
    assert type(info.value) is exc, "the exact type: a ValueError where today's is a RuntimeError is another behaviour"


# ---- one definition ---------------------------------------------------------------------------------------------------------------

def _without_docstrings(module) -> str:
    return re.sub(r'""".*?"""', "", inspect.getsource(module), flags=re.S)


def test_front_end_has_one_definition():
    """what the forms share is written once in ccvpe_amd.models: the stored-map check, the eval guard (once per wording), the rule
    that a call with one result returns it bare; and the trackers choose their update method in one place"""
    src = inspect.getsource(models)
    assert src.count("must be [B,512,512] or [B,1,512,512]") == 1
    assert src.count("call .eval() first") <= 2
    assert len(re.findall(r'call \.eval\(\) first"', src)) <= 1 and len(re.findall(r"call \.eval\(\) first \"", src)) <= 1
    # the tuple-or-bare rule: _launch alone decides it, and every call into the library goes through _launch or has no result to shape
    rule = re.findall(r"\bres\[0\] if\b|\belse res\[0\]", src)
    assert len(rule) == 1, rule
    launch = inspect.getsource(models._CVMBase._launch)
    assert len(re.findall(r"\bres\[0\] if\b|\belse res\[0\]", launch)) == 1
    for gone in ("_logits_call", "_alloc_rows", "_credible_alloc"):
        assert not hasattr(models._CVMBase, gone), gone
    code = _without_docstrings(aerial)
    assert len(re.findall(r"\blocalize_heading_prior_cached\b", code)) == 1
    assert len(re.findall(r"res\[-1\]", code)) == 1, "the trackers unpack an update's results in one place"


# ---- public surface ---------------------------------------------------------------------------------------------------------------
# sha256(signature, newline, docstring)[:12] of every public method, recorded before the front end was consolidated

SURFACE = {
    models._CVMBase: {
        "belief_credible": "7c52d4b6fc2b", "belief_summary": "71013a17109e", "encode_aerial": "466e241df1c9",
        "encode_ground": "785d9812990e", "evaluate": "143311d6cba6", "export_tuning": "123da822b98f", "forward": "5ecbf13b43ce",
        "forward_cached": "ba064c6b7a70", "heading_predict": "cc55bc721a48", "heading_prior_map": "ed5993a55ab2",
        "load_state_dict": "9062ced09106", "localize": "4cb20091c27f", "localize_cached": "1df74e291dfc",
        "localize_credible": "605e1e3a5285", "localize_credible_cached": "f99edbcdc139", "localize_heading": "bae00b082046",
        "localize_heading_cached": "b1d4cf030fc0", "localize_heading_prior": "8f3753617ec1",
        "localize_heading_prior_cached": "a1e7cd07a308", "localize_prior": "6ff556b5c216", "localize_prior_cached": "9e429a66ef03",
        "localize_region": "c07cf5d8c8b0", "localize_region_prior": "12f63d55f6dd", "localize_summary": "13082dfbd685",
        "localize_summary_cached": "d420542d00d3", "localize_topk": "357d0f17853c", "localize_topk_cached": "7b91e0879116",
        "postprocess": "c82a84ecc063", "postprocess_credible": "2ee6b0e576c4", "postprocess_heading": "10cf3c1419ff",
        "postprocess_prior": "59561c495416", "postprocess_rows": "b82a24d91a77", "postprocess_summary": "9b6d2393c54c",
        "postprocess_topk": "887e9479800a", "profile": "003cedde9c0a", "read_tap": "d690eb673ce3", "refresh_weights": "a27fb8dbebed",
        "set_debug": "f48876ac10b7", "set_streams": "292ed27b8cc5", "track_predict": "bfafddbb9bae", "track_predict_affine": "82eabd2ae0f7",
        "track_update": "408b50f5484a", "track_update_cached": "e78ba668c511", "track_update_logits": "e2b020ee8559",
    },
    aerial.Tracker: {"reset": "9e13548918b0", "step": "d87d561b71c8"},
    aerial.AffineTracker: {"reset": "9e13548918b0", "step": "3d9a3fff8d81"},
}


def _surface(cls):
    out = {}
    for name in vars(cls):
        f = getattr(cls, name)
        if not name.startswith("_") and callable(f):
            out[name] = hashlib.sha256(f"{inspect.signature(f)}\n{inspect.getdoc(f)}".encode()).hexdigest()[:12]
    return out


@pytest.mark.parametrize("cls", list(SURFACE), ids=lambda c: c.__name__)
def test_public_surface_is_unchanged(cls):
    got = _surface(cls)
    assert sorted(got) == sorted(SURFACE[cls]), "a public method was added, removed or renamed"
    changed = [n for n in got if got[n] != SURFACE[cls][n]]
    assert not changed, f"signature or docstring changed: {changed}"
