// Predict of the joint position-heading filter under an affine map per SOURCE heading bin (ccvpe_track_joint_predict_affine,
// DESIGN.md 4.30): the joint filter's predict (kernels_track_joint.hip) when the next frame's grid is a rotated,
// rescaled or sheared view of the last one (KITTI's heading-up tiles).  Per query, M[k'] = matrix[b][k'] a float64 matrix that maps an
// OUTPUT pixel index to the SOURCE index position bin k' reads (the convention of ccvpe_track_predict_affine):
//
//     A(k', .)  = track_predict_affine_kernel's c for the map joint[k'], the matrix M[k'] and taps   (|det| included, before floor, log)
//     prior     = track_joint_mix_kernel's C + floor over these A                                  (o, f, M[d], the chain: unchanged)
//
// Two launches:
//   track_joint_xy_affine_kernel  (256 tiles, B * nb)  slice s = b * nb + k': the sampling stage of track_predict_affine_kernel,
//                                                      statement for statement, with matrix + s * 6 and the taps of query s / nb,
//                                                      then track_blur.h's passes; c stored to `work`
//   track_joint_mix_kernel        (1024 groups, B)     kernels_track_joint.hip's, unedited (launch_track_joint_mix)
// The sampling and the passes are the affine position kernel's, so a slice of `work` holds that kernel's c bit for bit, and the matrix
// (1, 0, -dx, 0, 1, -dy) with integer dx, dy gives track_joint_xy_kernel's bits.  LDS as track_predict_affine_kernel:
// 4 * (S * 32 + S * (S + 1) + 2r + 7) bytes, S = 32 + 2r.  Every global read is bounds-checked against the grid, and the integer parts
// are clamped (NaN included) before they are converted, so no matrix moves a read outside the slice.  Nothing is accumulated with
// atomics: the same inputs give the same bits, alone as in a batch.
#include "track_blur.h"

namespace ccvpe {

__global__ __launch_bounds__(256) void track_joint_xy_affine_kernel(const TrackJointPredictAffineParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ja_smem[];
    constexpr int HW = TAIL_HW, n = HW * HW;
    const int s = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;    // slice s = b * nb + k'
    const int r = p.radius, S = affine_side(r), P = affine_pitch(r), WL = affine_wlen(r);
    const int b = s / p.nb;
    const int Y0 = (t / (HW / TRACK_T)) * TRACK_T, X0 = (t % (HW / TRACK_T)) * TRACK_T;
    float* mid = reinterpret_cast<float*>(ja_smem);   // [S][32] x-pass result (16-byte aligned rows)
    float* wt = mid + S * TRACK_T;                      // [WL] wt[3 + k] = t[|k - r|], k = 0 .. 2r
    float* src = wt + WL;                            // [S][P] samples s
    if (tid < WL) {
        const int k = tid - 3;
        const float* taps = p.taps + (size_t)b * p.taps_stride;
        wt[tid] = k >= 0 && k <= 2 * r ? taps[k < r ? r - k : k - r] : 0.f;
    }
    const double* M = p.matrix + (size_t)s * 6;
    const double m0 = M[0], m1 = M[1], m2 = M[2], m3 = M[3], m4 = M[4], m5 = M[5];
    const float det = (float)fabs(m0 * m4 - m1 * m3);
    // samples at output positions (X0 - r + lx, Y0 - r + ly): consecutive threads along a row, rows in turn
    const float* bel = p.joint + (size_t)s * n;
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
    const float4 c = track_blur_passes<0>(src, S, P, mid, wt, wt, r);
    const int cell = (Y0 + (tid >> 3)) * HW + X0 + (tid & 7) * 4;
    *reinterpret_cast<float4*>(p.work + (size_t)s * n + cell) = c;
}

void launch_track_joint_predict_affine(const TrackJointPredictAffineParams& p, hipStream_t s) {
    const size_t lds = affine_lds_bytes(p.radius);
    static LdsAttr attr;
    ensure_dynamic_lds(attr, reinterpret_cast<const void*>(track_joint_xy_affine_kernel), lds);
    CCVPE_LAUNCH(track_joint_xy_affine_kernel, dim3(TRACK_TILES, p.B * p.nb), dim3(256), lds, s, p);
    TrackJointPredictParams mix{};
    mix.turn_deg = p.turn_deg; mix.htaps = p.htaps; mix.htaps_stride = p.htaps_stride; mix.hradius = p.hradius; mix.floor = p.floor;
    mix.work = p.work; mix.prior = p.prior; mix.B = p.B; mix.nb = p.nb;
    launch_track_joint_mix(mix, s);
}

}  // namespace ccvpe
