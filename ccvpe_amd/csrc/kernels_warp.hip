// Device-side aerial preparation of the KITTI test loop: a chain of Pillow affine resamplings + center crop + ToTensor +
// Normalize.
//
// Reference: SatGrdDatasetTest.__getitem__ (datasets.py:577-598) runs sat.rotate(-heading) (NEAREST), two
// transform(AFFINE, BILINEAR) shifts (camera-GPS offset, test-split shift) and rotate(theta * rotation_range) (NEAREST) on the
// satellite tile, then TF.center_crop(512) and satmap_transform (train_KITTI.py:60-64; its Resize is a copy at 512^2).
// Each stage restates Pillow's libImaging/Geometry.c for an RGB image:
//   NEAREST  (affine_fixed): 16.16 fixed point, A = FIX(m0, m1, m3, m4), A2 = FIX(m2 + m0*.5 + m1*.5), A5 likewise,
//            FIX(v) = floor(v * 65536 + .5); pixel (x, y) reads in[(A5 + x*A3 + y*A4) >> 16][(A2 + x*A0 + y*A1) >> 16], 0 outside.
//            Pillow takes this path whenever the canvas corners map inside +-32768 (always, for rotations about the centre of
//            a canvas up to 16384); Image.rotate's shortcuts (copy, transposes) give the same bytes as this path fed its matrix.
//   BILINEAR (generic transform, double): xin = m0*(x+.5) + m1*(y+.5) + m2, yin likewise; 0 unless 0 <= xin < W and
//            0 <= yin < H; then xin -= .5, yin -= .5, columns clamp(floor(xin)) and clamp(floor(xin)+1), row clamp(floor(yin))
//            gives v1, row floor(yin)+1 gives v2 (v2 = v1 below the canvas), v = v1 + (v2-v1)*dy, stored as (uint8)v (truncated).
// Stages pass uint8 canvases to each other.  The kernel keeps none: one thread per output pixel walks the chain backwards and
// recomputes the intermediate values it needs (KITTI: 16 source pixels and 5 bilinear evaluations per output pixel).  The
// build passes -ffp-contract=off, so every double expression is evaluated as written, as Pillow's C is.
#include <math.h>

#include "kernels.h"

namespace ccvpe {

__device__ __forceinline__ long long warp_fix16(double v) { return (long long)floor(v * 65536.0 + 0.5); }

// value (3 channels) of stage S's output canvas at pixel (x, y), 0 <= x < W, 0 <= y < H; stage -1 is the source image
// fx[s]: the fixed-point coefficients A0..A5 of NEAREST stage s, computed once per thread (a stage near the source is visited
// up to 16 times per output pixel)
template <unsigned BIL, int S>
__device__ __forceinline__ void warp_at(const unsigned char* __restrict__ src, const double* __restrict__ m, const long long (*fx)[6],
                                        int H, int W, int x, int y, int* v) {
    if constexpr (S < 0) {
        const unsigned char* q = src + ((size_t)y * W + x) * 3;
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
    } else if constexpr (((BIL >> S) & 1u) == 0u) {
        const long long a0 = fx[S][0], a1 = fx[S][1], a2 = fx[S][2], a3 = fx[S][3], a4 = fx[S][4], a5 = fx[S][5];
        const long long xi = (a2 + (long long)y * a1 + (long long)x * a0) >> 16;   // Pillow accumulates the same sums in int
        const long long yi = (a5 + (long long)y * a4 + (long long)x * a3) >> 16;
        if (xi < 0 || xi >= W || yi < 0 || yi >= H) { v[0] = v[1] = v[2] = 0; return; }
        warp_at<BIL, S - 1>(src, m, fx, H, W, (int)xi, (int)yi, v);
    } else {
        const double* a = m + 6 * S;
        const double xo = (double)x + 0.5, yo = (double)y + 0.5;
        double xin = a[0] * xo + a[1] * yo + a[2];
        double yin = a[3] * xo + a[4] * yo + a[5];
        if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) { v[0] = v[1] = v[2] = 0; return; }   // NaN: outside
        xin -= 0.5;
        yin -= 0.5;
        const int xf = (int)floor(xin), yf = (int)floor(yin);
        const double dx = xin - (double)xf, dy = yin - (double)yf;
        const int x0 = xf < 0 ? 0 : xf, x1 = xf + 1 < W ? xf + 1 : W - 1, y0 = yf < 0 ? 0 : yf;
        int p[3], q[3];
        double v1[3], v2[3];
        warp_at<BIL, S - 1>(src, m, fx, H, W, x0, y0, p);
        warp_at<BIL, S - 1>(src, m, fx, H, W, x1, y0, q);
#pragma unroll
        for (int c = 0; c < 3; ++c) v1[c] = (double)p[c] + (double)(q[c] - p[c]) * dx;
        if (yf + 1 < H) {
            warp_at<BIL, S - 1>(src, m, fx, H, W, x0, yf + 1, p);
            warp_at<BIL, S - 1>(src, m, fx, H, W, x1, yf + 1, q);
#pragma unroll
            for (int c = 0; c < 3; ++c) v2[c] = (double)p[c] + (double)(q[c] - p[c]) * dx;
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) v2[c] = v1[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (int)(v1[c] + (v2[c] - v1[c]) * dy);
    }
}

// block = 64 x 4 output pixels of one sample (2-D tiles keep the rotated source footprint of a block compact);
// grid = (ceil(out_w / 64), ceil(out_h / 4), B)
template <unsigned BIL, int N>
__global__ __launch_bounds__(256) void warp_kernel(const WarpParams p) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int b = blockIdx.z;
    if (x >= p.out_w || y >= p.out_h) return;
    const unsigned char* src = p.in + (size_t)b * p.H * p.W * 3;
    const double* m = p.mat + (size_t)b * N * 6;
    long long fx[N][6];
#pragma unroll
    for (int s = 0; s < N; ++s) {
        if ((BIL >> s) & 1u) continue;
        const double* a = m + 6 * s;
        fx[s][0] = warp_fix16(a[0]); fx[s][1] = warp_fix16(a[1]); fx[s][3] = warp_fix16(a[3]); fx[s][4] = warp_fix16(a[4]);
        fx[s][2] = warp_fix16(a[2] + a[0] * 0.5 + a[1] * 0.5);
        fx[s][5] = warp_fix16(a[5] + a[3] * 0.5 + a[4] * 0.5);
    }
    int v[3];
    warp_at<BIL, N - 1>(src, m, fx, p.H, p.W, x + p.left, y + p.top, v);
    const size_t plane = (size_t)p.out_h * p.out_w;          // ToTensor + Normalize: the float stage of resize_v_kernel
    float* o = p.out + (size_t)b * 3 * plane + (size_t)y * p.out_w + x;
    o[0] = ((float)v[0] / 255.0f - p.mean[0]) / p.stdv[0];
    o[plane] = ((float)v[1] / 255.0f - p.mean[1]) / p.stdv[1];
    o[2 * plane] = ((float)v[2] / 255.0f - p.mean[2]) / p.stdv[2];
}

// every chain of 1..4 stages with at most 2 BILINEAR ones (bit s of BIL = stage s)
#define WARP_CASES(X)                                                                                                  \
    X(1, 0) X(1, 1)                                                                                                    \
    X(2, 0) X(2, 1) X(2, 2) X(2, 3)                                                                                    \
    X(3, 0) X(3, 1) X(3, 2) X(3, 4) X(3, 3) X(3, 5) X(3, 6)                                                            \
    X(4, 0) X(4, 1) X(4, 2) X(4, 4) X(4, 8) X(4, 3) X(4, 5) X(4, 6) X(4, 9) X(4, 10) X(4, 12)

int launch_warp(const WarpParams& p, hipStream_t s) {
    const dim3 grid((p.out_w + 63) / 64, (p.out_h + 3) / 4, p.B);
    switch (p.n * 16 + (int)p.bilinear) {
#define WARP_CASE(N, BIL) \
    case N * 16 + BIL: CCVPE_LAUNCH((warp_kernel<BIL##u, N>), grid, dim3(256), 0, s, p); return 0;
        WARP_CASES(WARP_CASE)
#undef WARP_CASE
        default: return -1;
    }
}

}  // namespace ccvpe
