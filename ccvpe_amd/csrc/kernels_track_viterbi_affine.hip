// MAP trajectory of a stream tracked across rotated frames (ccvpe_track_viterbi_affine, ccvpe_track_viterbi_back_affine, DESIGN.md
// 4.24): kernels_track_viterbi.hip's sweep behind a ccvpe_track_predict_affine call.  The affine move is itself a mixture - over the
// sample position y the blur reads and over which of that sample's four bilinear taps carried the mass - and both are read as latent
// choices, as 4.23 reads "move or floor".  Per query, with (ix, iy), the weights wx_a, wy_b and det of plane position y exactly as
// track_predict_affine_kernel computes them:
//
//     prior = Paff(b-; M) + floor                        the bits track_predict_affine_kernel takes the logf of
//     lik   = b > 0 ? b / prior : 0
//     q(y)  = max over the four taps of fl(det * fl(wy_b * fl(wx_a * v-(ix + a, iy + b))))
//     win   = max_ky fl(t[|ky - r|] * max_kx fl(t[|kx - r|] * q(x' - r + kx, y' - r + ky)))
//     m, w, W, e, score, stats                           kernels_track_viterbi.hip's lines
//
// The recursion only gathers: no adjoint, no reach rule.  Rounding is monotone and every factor is non-negative, so the step's "max, then
// multiply" and the backtrack's "multiply, then max" pick the same value.
//   track_viterbi_affine_step_kernel  (256 tiles, B)  the affine predict's sampling loop on b- and its two blur passes, then the same
//                                                     loop on v- with the largest of the four tap products in place of their sum and
//                                                     the two max passes over the 2r + 1 symmetric taps; w to `score`, the tile's
//                                                     (max, first index) to `work`.  A restart skips the second half.
//   track_viterbi_scale_kernel        (64 chunks, B)  kernels_track_viterbi.hip's, through launch_track_viterbi_scale
//   track_viterbi_back_affine_kernel  (B)             the 4 (2r + 1)^2 (sample, tap) pairs of one cell straight from global memory
// The sampling loop is written once (affine_tile_samples) and takes how the four taps combine, and the coordinates of a position are
// one function (affine_taps) for the step and the backtrack, so the arithmetic of prior, q and the candidates cannot drift apart.
// LDS is the affine predict's, affine_lds_bytes(r).  No atomics, no counters: the launch boundary is the hand-off, through `work`.
#include "tail_shared.h"
#include "track_maxmul.h"

namespace ccvpe {

// One query's matrix as the kernels hold it, and one plane position's sample: track_predict_affine_kernel's statements
struct AffineMap { double m0, m1, m2, m3, m4, m5; float det; };
__device__ __forceinline__ AffineMap affine_map(const double* matrix, int b) {
    const double* M = matrix + (size_t)b * 6;
    AffineMap a{M[0], M[1], M[2], M[3], M[4], M[5], 0.f};
    a.det = (float)fabs(a.m0 * a.m4 - a.m1 * a.m3);
    return a;
}
struct AffineTaps { int ix, iy; float wx0, wx1, wy0, wy1; };
__device__ __forceinline__ AffineTaps affine_taps(const AffineMap& a, double X, double Y) {
    const double sx = fma(a.m0, X, fma(a.m1, Y, a.m2)), sy = fma(a.m3, X, fma(a.m4, Y, a.m5));
    const double flx = floor(sx), fly = floor(sy);
    AffineTaps t;
    // integer parts clamped to +-2048 (beyond the grid either way; fmax returns the clamp for NaN): the conversion is defined
    t.ix = (int)fmin(fmax(flx, -2048.), 2048.); t.iy = (int)fmin(fmax(fly, -2048.), 2048.);
    const float fx = (float)(sx - flx), fy = (float)(sy - fly);
    t.wx0 = 1.f - fx; t.wx1 = fx; t.wy0 = 1.f - fy; t.wy1 = fy;
    return t;
}

// how a sample's four taps combine: the bilinear sum of the predict, or the largest single tap product
struct TapSum {
    __device__ __forceinline__ float operator()(float det, const AffineTaps& t, float v00, float v01, float v10, float v11) const {
        return det * (t.wy0 * (t.wx0 * v00 + t.wx1 * v01) + t.wy1 * (t.wx0 * v10 + t.wx1 * v11));
    }
};
__device__ __forceinline__ float affine_cand(float det, float wx, float wy, float v) { return det * (wy * (wx * v)); }
struct TapMax {
    __device__ __forceinline__ float operator()(float det, const AffineTaps& t, float v00, float v01, float v10, float v11) const {
        float q = maxmul_take(0.f, affine_cand(det, t.wx0, t.wy0, v00));
        q = maxmul_take(q, affine_cand(det, t.wx1, t.wy0, v01));
        q = maxmul_take(q, affine_cand(det, t.wx0, t.wy1, v10));
        return maxmul_take(q, affine_cand(det, t.wx1, t.wy1, v11));
    }
};

// Every thread of the workgroup: the S x S samples of map [512][512] at output positions (X0 - r + lx, Y0 - r + ly) into src [S][P],
// consecutive threads along a row, rows in turn - track_predict_affine_kernel's loop.  Every global read is bounds-checked against the
// grid, and the integer parts are clamped before they are converted, so no matrix moves a read outside the map.
template <class Combine>
__device__ __forceinline__ void affine_tile_samples(float* src, int S, int P, const AffineMap& a, const float* map, int r, int Y0, int X0,
                                                    Combine combine) {
    constexpr int HW = TAIL_HW;
    const int tid = threadIdx.x;
    const int q = 256 / S, rem = 256 - q * S;
    int ly = tid / S, lx = tid - ly * S;
    for (int i = tid; i < S * S; i += 256) {
        const AffineTaps t = affine_taps(a, (double)(X0 - r + lx), (double)(Y0 - r + ly));
        const int ix = t.ix, iy = t.iy;
        const bool r0 = (unsigned)iy < (unsigned)HW, r1 = (unsigned)(iy + 1) < (unsigned)HW;
        const bool c0 = (unsigned)ix < (unsigned)HW, c1 = (unsigned)(ix + 1) < (unsigned)HW;
        const float v00 = r0 && c0 ? map[iy * HW + ix] : 0.f;
        const float v01 = r0 && c1 ? map[iy * HW + ix + 1] : 0.f;
        const float v10 = r1 && c0 ? map[(iy + 1) * HW + ix] : 0.f;
        const float v11 = r1 && c1 ? map[(iy + 1) * HW + ix + 1] : 0.f;
        src[ly * P + lx] = combine(a.det, t, v00, v01, v10, v11);
        lx += rem; ly += q;
        if (lx >= S) { lx -= S; ++ly; }
    }
}

__global__ __launch_bounds__(256) void track_viterbi_affine_step_kernel(const TrackViterbiAffineParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char va_smem[];
    __shared__ float redv[4];
    __shared__ int redi[4];
    constexpr int HW = TAIL_HW, n = HW * HW;
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const int r = p.radius, S = affine_side(r), P = affine_pitch(r), WL = affine_wlen(r);
    const int Y0 = (t / (HW / TRACK_T)) * TRACK_T, X0 = (t % (HW / TRACK_T)) * TRACK_T;
    const int cell = (Y0 + (tid >> 3)) * HW + X0 + (tid & 7) * 4;
    float* mid = reinterpret_cast<float*>(va_smem);   // [S][32] x-pass result (16-byte aligned rows)
    float* wt = mid + S * TRACK_T;                    // [WL] wt[3 + k] = t[|k - r|], k = 0 .. 2r
    float* src = wt + WL;                             // [S][P] samples
    if (tid < WL) {
        const int k = tid - 3;
        const float* taps = p.taps + (size_t)b * p.taps_stride;
        wt[tid] = k >= 0 && k <= 2 * r ? taps[k < r ? r - k : k - r] : 0.f;
    }
    const AffineMap a = affine_map(p.matrix, b);
    float4 w = *reinterpret_cast<const float4*>(p.belief + (size_t)b * n + cell);
    affine_tile_samples(src, S, P, a, p.belief_prev + (size_t)b * n, r, Y0, X0, TapSum());
    __syncthreads();
    const float4 c = track_blur_passes<0>(src, S, P, mid, wt, wt, r);
    const float fl = p.floor[b];
    w.x = w.x > 0.f ? w.x / (c.x + fl) : 0.f;
    w.y = w.y > 0.f ? w.y / (c.y + fl) : 0.f;
    w.z = w.z > 0.f ? w.z / (c.z + fl) : 0.f;
    w.w = w.w > 0.f ? w.w / (c.w + fl) : 0.f;
    const int j = viterbi_prev_index(p.prev_stats, b);
    const float peak = j >= 0 ? p.score_prev[(size_t)b * n + j] : 0.f;
    if (peak > 0.f) {                       // the same for every thread of the query; else a restart: m = 1
        __syncthreads();                    // the y pass has read mid
        affine_tile_samples(src, S, P, a, p.score_prev + (size_t)b * n, r, Y0, X0, TapMax());
        __syncthreads();
        const float4 win = track_maxmul_passes<0>(src, S, P, mid, wt, wt, r);
        const float jump = fl * peak;
        w.x = w.x * (jump > win.x ? jump : win.x);
        w.y = w.y * (jump > win.y ? jump : win.y);
        w.z = w.z * (jump > win.z ? jump : win.z);
        w.w = w.w * (jump > win.w ? jump : win.w);
    }
    w = make_float4(viterbi_clean(w.x), viterbi_clean(w.y), viterbi_clean(w.z), viterbi_clean(w.w));
    *reinterpret_cast<float4*>(p.score + (size_t)b * n + cell) = w;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    argmax_merge(best, bi, w.x, cell);
    argmax_merge(best, bi, w.y, cell + 1);
    argmax_merge(best, bi, w.z, cell + 2);
    argmax_merge(best, bi, w.w, cell + 3);
    argmax_wave(best, bi);
    if ((tid & 63) == 0) { redv[tid >> 6] = best; redi[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < 4; ++v) argmax_merge(best, bi, redv[v], redi[v]);
        float* wk = p.work + (size_t)b * VITERBI_WORK_FLOATS;
        wk[t] = best;
        wk[TRACK_TILES + t] = __int_as_float(bi);
    }
}

void launch_track_viterbi_affine(const TrackViterbiAffineParams& p, hipStream_t s) {
    TrackViterbiParams v{};
    v.belief = p.belief; v.belief_prev = p.belief_prev; v.score_prev = p.score_prev; v.prev_stats = p.prev_stats;
    v.score = p.score; v.stats = p.stats; v.work = p.work; v.B = p.B;
    if (!p.belief_prev) {                   // a stream's first frame has no motion: the translation form's two launches themselves
        launch_track_viterbi(v, s);
        return;
    }
    const size_t lds = affine_lds_bytes(p.radius);
    static LdsAttr step_attr;
    ensure_dynamic_lds(step_attr, reinterpret_cast<const void*>(track_viterbi_affine_step_kernel), lds);
    CCVPE_LAUNCH(track_viterbi_affine_step_kernel, dim3(TRACK_TILES, p.B), dim3(256), lds, s, p);
    launch_track_viterbi_scale(v, s);
}

// One link of the backtrack.  One workgroup per query; thread tid takes sample positions tid, tid + 256, .. of the (2r + 1)^2 window of
// `cell` in raster order and weighs the four taps of each, fl(t_y * fl(t_x * cand)); a pair whose source cell lies outside the grid is
// no candidate.  The largest wins, on ties the smallest source cell index, whatever sample it came through.  Every read is guarded: j
// by viterbi_prev_index, cell against the grid, a tap's source against the grid.
__global__ __launch_bounds__(256) void track_viterbi_back_affine_kernel(const TrackViterbiBackAffineParams p) {
    __shared__ float redv[4];
    __shared__ int redi[4];
    constexpr int HW = TAIL_HW, n = HW * HW;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int cell = p.cell[b];
    const int j = viterbi_prev_index(p.prev_stats, b);
    int* out = p.back + (size_t)b * 2;
    if ((unsigned)cell >= (unsigned)n || j < 0) {       // the end of a backtrack or the frame behind a broken one; no j: nothing to point at
        if (tid == 0) { out[0] = (unsigned)cell >= (unsigned)n ? j : -1; out[1] = VITERBI_LINK_START; }
        return;
    }
    const int r = p.radius, K = 2 * r + 1;
    const float* prev = p.score_prev + (size_t)b * n;
    const float* taps = p.taps + (size_t)b * p.taps_stride;
    const AffineMap a = affine_map(p.matrix, b);
    const int x0 = cell % HW - r, y0 = cell / HW - r;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = tid; i < K * K; i += 256) {
        const int ky = i / K, kx = i - ky * K;
        const float tx = taps[kx < r ? r - kx : kx - r], ty = taps[ky < r ? r - ky : ky - r];
        const AffineTaps t = affine_taps(a, (double)(x0 + kx), (double)(y0 + ky));
        const int ix = t.ix, iy = t.iy;
        const bool r0 = (unsigned)iy < (unsigned)HW, r1 = (unsigned)(iy + 1) < (unsigned)HW;
        const bool c0 = (unsigned)ix < (unsigned)HW, c1 = (unsigned)(ix + 1) < (unsigned)HW;
        if (r0 && c0) argmax_merge(best, bi, ty * (tx * affine_cand(a.det, t.wx0, t.wy0, prev[iy * HW + ix])), iy * HW + ix);
        if (r0 && c1) argmax_merge(best, bi, ty * (tx * affine_cand(a.det, t.wx1, t.wy0, prev[iy * HW + ix + 1])), iy * HW + ix + 1);
        if (r1 && c0) argmax_merge(best, bi, ty * (tx * affine_cand(a.det, t.wx0, t.wy1, prev[(iy + 1) * HW + ix])), (iy + 1) * HW + ix);
        if (r1 && c1) argmax_merge(best, bi, ty * (tx * affine_cand(a.det, t.wx1, t.wy1, prev[(iy + 1) * HW + ix + 1])), (iy + 1) * HW + ix + 1);
    }
    argmax_wave(best, bi);
    if ((tid & 63) == 0) { redv[tid >> 6] = best; redi[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < 4; ++v) argmax_merge(best, bi, redv[v], redi[v]);
        const float jump = p.floor[b] * prev[j];
        if (!(best > 0.f) && !(jump > 0.f)) { out[0] = j; out[1] = VITERBI_LINK_START; }
        else if (jump > best) { out[0] = j; out[1] = VITERBI_LINK_JUMP; }
        else { out[0] = bi; out[1] = VITERBI_LINK_MOVE; }
    }
}

void launch_track_viterbi_back_affine(const TrackViterbiBackAffineParams& p, hipStream_t s) {
    CCVPE_LAUNCH(track_viterbi_back_affine_kernel, dim3(p.B), dim3(256), 0, s, p);
}

}  // namespace ccvpe
