// Motion update of a position belief under an affine map (ccvpe_track_predict_affine): the predict half of the histogram
// filter when the next frame's grid is a rotated, rescaled or sheared view of the last one (KITTI's heading-up tiles, a zoom change).
// Per query, with the belief B extended by zero outside its 512 x 512 grid and M = (m0..m5) a float64 matrix that maps an OUTPUT pixel
// index to the SOURCE index position it reads (B[j][i] sits at (i, j)):
//
//     (sx, sy)  = (m0 x + m1 y + m2, m3 x + m4 y + m5)                        float64: fma(m0, x, fma(m1, y, m2))
//     s(x, y)   = |m0 m4 - m1 m3| * bilinear sample of B at (sx, sy)          on the infinite plane
//     c         = s convolved with t[|i|], i = -r..r, along x, then along y
//     out(x, y) = logf(c(x, y) + floor)                                       for the 512 x 512 window
//
// The sample: ix = floor(sx), fx = (float)(sx - ix) rounded once, weights (1.f - fx, fx), likewise along y, and
// s = det * (wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11)) in float32 with det = (float)|m0 m4 - m1 m3|; every term is
// non-negative and a fraction of exactly 0 weighs the one source pixel with exactly 1.  A pass is 2r + 1 fused multiply-adds in ascending
// source index from a zero accumulator - the order of track_predict_kernel, whose extra first term is an exact 0 * v - so the matrix
// (1, 0, -dx, 0, 1, -dy) with integer dx, dy gives that kernel's bits.
//
// Grid (256 tiles, B): a workgroup owns a 32 x 32 output tile.  It evaluates s on the S x S positions its tile's blur reaches
// (S = 32 + 2r) straight from global memory - the 1 MB belief is L2-resident and neighbouring samples share their source pixels through
// the caches; the rotated footprint is not staged - and writes them to LDS at an odd row pitch; the x pass runs out of that into an
// [S][32] buffer and the y pass out of that, one float4 of output per thread, as in track_predict_kernel.  LDS:
// 4 * (S * 32 + S * (S + 1) + 2r + 7) bytes: 13.6 KB at r = 6, 49.8 KB at r = 32 - three workgroups per CU at the largest radius.  Every
// global read is bounds-checked against the grid, and the integer parts are clamped (NaN included) before they are converted, so no
// matrix moves a read outside the tensors.
#include "track_blur.h"

namespace ccvpe {

__global__ __launch_bounds__(256) void track_predict_affine_kernel(const TrackPredictAffineParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ta_smem[];
    constexpr int HW = TAIL_HW, n = HW * HW;
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const int r = p.radius, S = affine_side(r), P = affine_pitch(r), WL = affine_wlen(r);
    const int Y0 = (t / (HW / TRACK_T)) * TRACK_T, X0 = (t % (HW / TRACK_T)) * TRACK_T;
    float* mid = reinterpret_cast<float*>(ta_smem);   // [S][32] x-pass result (16-byte aligned rows)
    float* wt = mid + S * TRACK_T;                      // [WL] wt[3 + k] = t[|k - r|], k = 0 .. 2r
    float* src = wt + WL;                            // [S][P] samples s
    if (tid < WL) {
        const int k = tid - 3;
        const float* taps = p.taps + (size_t)b * p.taps_stride;
        wt[tid] = k >= 0 && k <= 2 * r ? taps[k < r ? r - k : k - r] : 0.f;
    }
    const double* M = p.matrix + (size_t)b * 6;
    const double m0 = M[0], m1 = M[1], m2 = M[2], m3 = M[3], m4 = M[4], m5 = M[5];
    const float det = (float)fabs(m0 * m4 - m1 * m3);
    // samples at output positions (X0 - r + lx, Y0 - r + ly): consecutive threads along a row, rows in turn
    const float* bel = p.belief + (size_t)b * n;
    const int q = 256 / S, rem = 256 - q * S;
    int ly = tid / S, lx = tid - ly * S;
    for (int i = tid; i < S * S; i += 256) {
        const double X = (double)(X0 - r + lx), Y = (double)(Y0 - r + ly);
        const double sx = fma(m0, X, fma(m1, Y, m2)), sy = fma(m3, X, fma(m4, Y, m5));
        const double flx = floor(sx), fly = floor(sy);
        // integer parts clamped to +-2048 (beyond the grid either way; fmax returns the clamp for NaN): the conversion is defined
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
    track_blur_store<0>(src, S, P, mid, wt, wt, r, p.floor, p.log_prior, b, Y0, X0);
}

void launch_track_predict_affine(const TrackPredictAffineParams& p, hipStream_t s) {
    const size_t lds = affine_lds_bytes(p.radius);
    static LdsAttr attr;
    ensure_dynamic_lds(attr, reinterpret_cast<const void*>(track_predict_affine_kernel), lds);
    CCVPE_LAUNCH(track_predict_affine_kernel, dim3(TRACK_TILES, p.B), dim3(256), lds, s, p);
}

}  // namespace ccvpe
