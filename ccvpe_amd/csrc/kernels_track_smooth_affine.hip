// Backward pass over stored beliefs behind an affine predict (ccvpe_track_smooth_affine): ccvpe_track_smooth for streams
// tracked through ccvpe_track_predict_affine (KITTI's heading-up tiles).  Per query, with b the filter posterior of frame t, s' the
// smoothed map of frame t + 1 and M, taps, floor the arguments of the ccvpe_track_predict_affine call that carried b into frame t + 1:
//
//     prior = Paff(b; M) + floor                        the bits track_predict_affine_kernel takes the logf of
//     g     = s' > 0 ? s' / prior : 0
//     G     = sum g
//     h(y)  = (g, zero-extended, convolved with t[|k|] along x, then y)(y)     for y in [-r, 511 + r]^2, 0 beyond
//     A(x)  = sum over y, rows ascending, then columns ascending, of  det * (wy_b * (wx_a * h(y)))       terms with wx_a * wy_b > 0
//     a     = fmaf(floor, G, A),   w = b * a,  Z = sum w,  s = w * (1 / Z)
//
// wx_a, wy_b are the float32 bilinear weights the predict's sample at plane position y gives source cell x - recomputed here with the
// predict's own expressions, so they are its bits.  The adjoint of the predict's gather is a scatter; it is taken as a gather instead:
// cell x walks the integer positions of the bounding box of the preimage of the open square (i - 1, i + 1) x (j - 1, j + 1) under M,
// rounded outward plus one position on every side, and rejects every position whose sample does not touch x.  Only positive terms
// enter the sum, in a fixed order, so any superset of the touching positions gives the same bits and nothing is accumulated with
// atomics.  Reach: a query is supported when det = (float)|m0 m4 - m1 m3| is finite and non-zero and the half extents of that box,
// hx = |N00| + |N01|, hy = |N10| + |N11| (N the float64 inverse of the linear part), are both <= 3; any other query is a broken link:
// g = 0, so G = 0 and the result is b itself (rule 1 of 4.20).
//
// Four launches, each grid-wide sum between two of them:
//   track_smooth_affine_ratio_kernel   (256 tiles, B)       the predict's sampling of b and its two passes; g stored to `work`, the
//                                                           tile's sum of g; an unsupported query stores zeros
//   track_smooth_affine_blur_kernel    (extended tiles, B)  h = blur(g) on the window plus r, to `work` at pitch 576, origin (32, 32)
//   track_smooth_affine_weight_kernel  (256 tiles, B)       G from the 256 tile sums; the gather, one float4 of cells per thread; w
//                                                           stored to `smoothed` (G == 0: b itself); the tile's sum of w, (max, index)
//   track_smooth_scale_kernel          (64 chunks, B)       kernels_track_smooth.hip's, on the same layout of `work`
// The sums have the orders of kernels_track_smooth.hip (track_smooth_work.h).  No counters: the launch boundaries are the hand-offs.
// `smoothed` may be `smoothed_next`: s' is read by the first launch only, and every cell by the thread that later writes it.
#include "tail_shared.h"
#include "track_blur.h"
#include "track_smooth_work.h"

namespace ccvpe {

// h: [576][576] floats per query behind every query's SMOOTH_WORK_FLOATS; plane position (x, y) sits at [y + 32][x + 32], whatever r
static constexpr int SMOOTH_H_PITCH = TAIL_HW + 2 * TRACK_MAX_R, SMOOTH_H_ORG = TRACK_MAX_R;
static constexpr size_t SMOOTH_H_FLOATS = (size_t)SMOOTH_H_PITCH * SMOOTH_H_PITCH;
size_t track_smooth_affine_work_bytes(int B) { return sizeof(float) * (SMOOTH_WORK_FLOATS + SMOOTH_H_FLOATS) * (size_t)B; }
__device__ __forceinline__ float* smooth_h(float* work, int B, int b) { return work + (size_t)B * SMOOTH_WORK_FLOATS + (size_t)b * SMOOTH_H_FLOATS; }

// the matrix of a query, its float32 |det| and the reach of its adjoint
struct SmoothAffine {
    double m0, m1, m2, m3, m4, m5;
    double n00, n01, n10, n11;   // inverse of the linear part
    double hx, hy;               // half extents of the candidate box
    float det;
    bool reach;
};
__device__ __forceinline__ SmoothAffine smooth_affine(const double* matrix, int b) {
    const double* M = matrix + (size_t)b * 6;
    SmoothAffine a;
    a.m0 = M[0]; a.m1 = M[1]; a.m2 = M[2]; a.m3 = M[3]; a.m4 = M[4]; a.m5 = M[5];
    const double d = a.m0 * a.m4 - a.m1 * a.m3;
    a.det = (float)fabs(d);
    a.n00 = a.m4 / d; a.n01 = -a.m1 / d; a.n10 = -a.m3 / d; a.n11 = a.m0 / d;
    a.hx = fabs(a.n00) + fabs(a.n01); a.hy = fabs(a.n10) + fabs(a.n11);
    // NaN fails every comparison
    a.reach = isfinite(a.det) && a.det != 0.f && a.hx <= 3. && a.hy <= 3.;
    return a;
}

__global__ __launch_bounds__(256) void track_smooth_affine_ratio_kernel(const TrackSmoothAffineParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ar_smem[];
    __shared__ float red[4];
    constexpr int HW = TAIL_HW, n = HW * HW;
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const int r = p.radius, S = affine_side(r), P = affine_pitch(r), WL = affine_wlen(r);
    const int Y0 = (t / (HW / TRACK_T)) * TRACK_T, X0 = (t % (HW / TRACK_T)) * TRACK_T;
    const SmoothWork wk = smooth_work(p.work, b);
    const int cell = (Y0 + (tid >> 3)) * HW + X0 + (tid & 7) * 4;
    const SmoothAffine A = smooth_affine(p.matrix, b);
    if (!A.reach) {   // the same for every thread of the query: a broken link
        if (tid == 0) wk.gsum[t] = 0.f;
        *reinterpret_cast<float4*>(wk.g + cell) = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    float* mid = reinterpret_cast<float*>(ar_smem);   // [S][32] x-pass result (16-byte aligned rows)
    float* wt = mid + S * TRACK_T;                      // [WL] wt[3 + k] = t[|k - r|], k = 0 .. 2r
    float* src = wt + WL;                               // [S][P] samples s
    if (tid < WL) {
        const int k = tid - 3;
        const float* taps = p.taps + (size_t)b * p.taps_stride;
        wt[tid] = k >= 0 && k <= 2 * r ? taps[k < r ? r - k : k - r] : 0.f;
    }
    // track_predict_affine_kernel's sampling, statement for statement: the prior is that kernel's bits
    const double m0 = A.m0, m1 = A.m1, m2 = A.m2, m3 = A.m3, m4 = A.m4, m5 = A.m5;
    const float det = A.det;
    const float* bel = p.belief + (size_t)b * n;
    const int q = 256 / S, rem = 256 - q * S;
    int ly = tid / S, lx = tid - ly * S;
    for (int i = tid; i < S * S; i += 256) {
        const double X = (double)(X0 - r + lx), Y = (double)(Y0 - r + ly);
        const double sx = fma(m0, X, fma(m1, Y, m2)), sy = fma(m3, X, fma(m4, Y, m5));
        const double flx = floor(sx), fly = floor(sy);
        const int ix = (int)fmin(fmax(flx, -2048.), 2048.), iy = (int)fmin(fmax(fly, -2048.), 2048.);
        const float fx = (float)(sx - flx), fy = (float)(sy - fly);
        const bool r0 = (unsigned)iy < (unsigned)HW, r1 = (unsigned)(iy + 1) < (unsigned)HW;
        const bool c0 = (unsigned)ix < (unsigned)HW, c1 = (unsigned)(ix + 1) < (unsigned)HW;
        const float v00 = r0 && c0 ? bel[iy * HW + ix] : 0.f;
        const float v01 = r0 && c1 ? bel[iy * HW + ix + 1] : 0.f;
        const float v10 = r1 && c0 ? bel[(iy + 1) * HW + ix] : 0.f;
        const float v11 = r1 && c1 ? bel[(iy + 1) * HW + ix + 1] : 0.f;
        const float wx0 = 1.f - fx, wx1 = fx, wy0 = 1.f - fy, wy1 = fy;
        src[ly * P + lx] = det * (wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11));
        lx += rem; ly += q;
        if (lx >= S) { lx -= S; ++ly; }
    }
    __syncthreads();
    const float4 c = track_blur_passes<0>(src, S, P, mid, wt, wt, r);
    const float fl = p.floor[b];
    const float4 sn = *reinterpret_cast<const float4*>(p.next + (size_t)b * n + cell);
    float4 g;
    g.x = sn.x > 0.f ? sn.x / (c.x + fl) : 0.f;
    g.y = sn.y > 0.f ? sn.y / (c.y + fl) : 0.f;
    g.z = sn.z > 0.f ? sn.z / (c.z + fl) : 0.f;
    g.w = sn.w > 0.f ? sn.w / (c.w + fl) : 0.f;
    *reinterpret_cast<float4*>(wk.g + cell) = g;
    const float s = smooth_wave_sum(((g.x + g.y) + g.z) + g.w);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) wk.gsum[t] = ((red[0] + red[1]) + red[2]) + red[3];
}

// tiles of 32 x 32 over the plane positions [-r, 511 + r]^2, per side
__host__ __device__ constexpr int smooth_ext_tiles(int r) { return (TAIL_HW + 2 * r + TRACK_T - 1) / TRACK_T; }

__global__ __launch_bounds__(256) void track_smooth_affine_blur_kernel(const TrackSmoothAffineParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ab_smem[];
    constexpr int HW = TAIL_HW;
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const int r = p.radius, S = affine_side(r), P = affine_pitch(r), WL = affine_wlen(r);
    const int nt = smooth_ext_tiles(r);
    const int Y0 = (t / nt) * TRACK_T - r, X0 = (t % nt) * TRACK_T - r;   // the tile's first plane position
    float* mid = reinterpret_cast<float*>(ab_smem);
    float* wt = mid + S * TRACK_T;
    float* src = wt + WL;
    if (tid < WL) {
        const int k = tid - 3;
        const float* taps = p.taps + (size_t)b * p.taps_stride;
        wt[tid] = k >= 0 && k <= 2 * r ? taps[k < r ? r - k : k - r] : 0.f;
    }
    // g at rows Y0 - r .. Y0 + 31 + r, columns X0 - r .. X0 + 31 + r, zeros outside the window: a wave per row, lanes along the row
    const float* g = smooth_work(p.work, b).g;
    const int gx0 = X0 - r, gy0 = Y0 - r;
    const int lane = tid & 63, wave = tid >> 6;
    for (int ly = wave; ly < S; ly += 4) {
        const int gy = gy0 + ly;
        const bool rowin = (unsigned)gy < (unsigned)HW;
        for (int lx = lane; lx < S; lx += 64) {
            const int gx = gx0 + lx;
            src[ly * P + lx] = rowin && (unsigned)gx < (unsigned)HW ? g[gy * HW + gx] : 0.f;
        }
    }
    __syncthreads();
    const float4 c = track_blur_passes<0>(src, S, P, mid, wt, wt, r);
    // positions within r of the window only: those are the ones the gather reads
    const int y = Y0 + (tid >> 3), x = X0 + (tid & 7) * 4, last = HW - 1 + r;
    if (y <= last) {
        float* row = smooth_h(p.work, p.B, b) + (size_t)(y + SMOOTH_H_ORG) * SMOOTH_H_PITCH + SMOOTH_H_ORG + x;
        if (x <= last) row[0] = c.x;
        if (x + 1 <= last) row[1] = c.y;
        if (x + 2 <= last) row[2] = c.z;
        if (x + 3 <= last) row[3] = c.w;
    }
}

__global__ __launch_bounds__(256) void track_smooth_affine_weight_kernel(const TrackSmoothAffineParams p) {
    __shared__ float red[4], redv[4], redG;
    __shared__ int redi[4];
    constexpr int HW = TAIL_HW, n = HW * HW;
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const int r = p.radius;
    const int Y0 = (t / (HW / TRACK_T)) * TRACK_T, X0 = (t % (HW / TRACK_T)) * TRACK_T;
    const SmoothWork wk = smooth_work(p.work, b);
    if (tid < 64) {
        const float G = smooth_sum_tiles(wk.gsum);
        if (tid == 0) redG = G;
    }
    __syncthreads();
    const int j = Y0 + (tid >> 3), i0 = X0 + (tid & 7) * 4;
    const int cell = j * HW + i0;
    const float fl = p.floor[b], G = redG;
    const float4 bq = *reinterpret_cast<const float4*>(p.belief + (size_t)b * n + cell);
    float4 w = bq;   // G == 0: the next map has no positive cell, or the link is out of reach; the result is the belief itself
    if (G != 0.f) {
        const SmoothAffine A = smooth_affine(p.matrix, b);
        const double m0 = A.m0, m1 = A.m1, m2 = A.m2, m3 = A.m3, m4 = A.m4, m5 = A.m5;
        const float det = A.det;
        // The candidates of cells i0 .. i0 + 3 of row j: the box around N ((i, j) - (m2, m5)) of half extents (hx, hy) for the first and
        // the last cell, rounded outward plus one position, clipped to where h lives.  Clamped before the conversion (fmax and fmin
        // return the clamp for NaN).  A supported query (hx, hy <= 3) has at most 19 positions per axis; the cap only bounds the loop.
        const double ux = (double)i0 - m2, uy = (double)j - m5;
        const double px = A.n00 * ux + A.n01 * uy, py = A.n10 * ux + A.n11 * uy;
        const double qx = px + 3. * A.n00, qy = py + 3. * A.n10;
        const double lo = (double)-r, hi = (double)(HW - 1 + r);
        const int x_lo = (int)fmin(fmax(floor(fmin(px, qx) - A.hx) - 1., lo), hi);
        const int y_lo = (int)fmin(fmax(floor(fmin(py, qy) - A.hy) - 1., lo), hi);
        const int x_hi = min((int)fmin(fmax(ceil(fmax(px, qx) + A.hx) + 1., lo), hi), x_lo + 20);
        const int y_hi = min((int)fmin(fmax(ceil(fmax(py, qy) + A.hy) + 1., lo), hi), y_lo + 20);
        const float* h = smooth_h(p.work, p.B, b);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (int yy = y_lo; yy <= y_hi; ++yy) {
            const double Y = (double)yy;
            const double bx = fma(m1, Y, m2), by = fma(m4, Y, m5);
            const float* hrow = h + (size_t)(yy + SMOOTH_H_ORG) * SMOOTH_H_PITCH + SMOOTH_H_ORG;
            for (int yx = x_lo; yx <= x_hi; ++yx) {
                // the predict's expressions for the sample at plane position (yx, yy)
                const double X = (double)yx;
                const double sx = fma(m0, X, bx), sy = fma(m3, X, by);
                const double flx = floor(sx), fly = floor(sy);
                const int ix = (int)fmin(fmax(flx, -2048.), 2048.), iy = (int)fmin(fmax(fly, -2048.), 2048.);
                const float fx = (float)(sx - flx), fy = (float)(sy - fly);
                const int rb = j - iy;            // 0: the sample's upper row, 1: its lower row
                if ((unsigned)rb > 1u) continue;
                const float wy = rb == 0 ? 1.f - fy : fy;
                const float hv = hrow[yx];
                const int ca = i0 - ix;           // cell i0 + c is column ca + c of the sample
                const float wx0 = 1.f - fx, wx1 = fx;
#define CCVPE_SMOOTH_TERM(acc, c)                                              \
                if ((unsigned)(ca + c) <= 1u) {                                \
                    const float wx = ca + c == 0 ? wx0 : wx1;                  \
                    if (wx * wy > 0.f) acc = acc + det * (wy * (wx * hv));     \
                }
                CCVPE_SMOOTH_TERM(a0, 0)
                CCVPE_SMOOTH_TERM(a1, 1)
                CCVPE_SMOOTH_TERM(a2, 2)
                CCVPE_SMOOTH_TERM(a3, 3)
#undef CCVPE_SMOOTH_TERM
            }
        }
        w.x = bq.x * fmaf(fl, G, a0);
        w.y = bq.y * fmaf(fl, G, a1);
        w.z = bq.z * fmaf(fl, G, a2);
        w.w = bq.w * fmaf(fl, G, a3);
    }
    float best = -INFINITY;
    int bi = 0x7fffffff;
    argmax_merge(best, bi, w.x, cell);
    argmax_merge(best, bi, w.y, cell + 1);
    argmax_merge(best, bi, w.z, cell + 2);
    argmax_merge(best, bi, w.w, cell + 3);
    argmax_wave(best, bi);
    const float s = smooth_wave_sum(((w.x + w.y) + w.z) + w.w);
    // (stored behind the reductions: no vector write stands in the slot behind the wide store, tests/test_isa_hazard.py)
    *reinterpret_cast<float4*>(p.smoothed + (size_t)b * n + cell) = w;
    if ((tid & 63) == 0) { red[tid >> 6] = s; redv[tid >> 6] = best; redi[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < 4; ++v) argmax_merge(best, bi, redv[v], redi[v]);
        wk.wsum[t] = ((red[0] + red[1]) + red[2]) + red[3];
        wk.wmax[t] = best;
        wk.widx[t] = __int_as_float(bi);
    }
}

void launch_track_smooth_affine(const TrackSmoothAffineParams& p, hipStream_t s) {
    const size_t lds = affine_lds_bytes(p.radius);
    const int nt = smooth_ext_tiles(p.radius);
    static LdsAttr ratio_attr, blur_attr;
    ensure_dynamic_lds(ratio_attr, reinterpret_cast<const void*>(track_smooth_affine_ratio_kernel), lds);
    ensure_dynamic_lds(blur_attr, reinterpret_cast<const void*>(track_smooth_affine_blur_kernel), lds);
    CCVPE_LAUNCH(track_smooth_affine_ratio_kernel, dim3(TRACK_TILES, p.B), dim3(256), lds, s, p);
    CCVPE_LAUNCH(track_smooth_affine_blur_kernel, dim3(nt * nt, p.B), dim3(256), lds, s, p);
    CCVPE_LAUNCH(track_smooth_affine_weight_kernel, dim3(TRACK_TILES, p.B), dim3(256), 0, s, p);
    TrackSmoothParams q{};
    q.smoothed = p.smoothed; q.stats = p.stats; q.work = p.work; q.B = p.B;
    launch_track_smooth_scale(q, s);
}

}  // namespace ccvpe
