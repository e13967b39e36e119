// Motion update of a position belief (ccvpe_track_predict): the predict half of a histogram filter over the 512 x 512
// output grid.  Per query, with the belief B extended by zero outside its grid:
//
//     s(x, y)   = bilinear sample of B at (x - dx, y - dy)
//     c         = s convolved with t[|i|], i = -r..r, along x, then along y
//     out(x, y) = logf(c(x, y) + floor)                       for the 512 x 512 window
//
// The shift is the same for every pixel of a query, so the bilinear sample is a separable 2-tap filter with weights (1 - f, f), f the
// fractional part of the shift, and each pass folds it into its blur: 2r + 2 merged weights
//
//     u[k] = f * t[|k - r|] + (1 - f) * t[|k - 1 - r|]        k = 0 .. 2r + 1   (t = 0 outside 0..r)
//
// over the source pixels q + k, q = x - floor(dx) - r - 1.  f == 0 gives u[k] = t[|k - 1 - r|] exactly (0 * t + 1 * t), so an integer
// shift weighs the one source pixel with exactly 1 times its tap.  All terms are non-negative; a pass is 2r + 2 fused multiply-adds.
//
// Grid (256 tiles, B): a workgroup owns a 32 x 32 output tile.  It stages the S x S source pixels its tile needs (S = 32 + 2r + 1, one
// coalesced read per row segment, zeros outside the grid) in LDS once, runs the x pass out of LDS into an [S][32] buffer in LDS and the
// y pass out of that, one float4 of output per thread.  LDS: 4 * (S * 32 + S * P + 2 * (2r + 8)) bytes, P = S or S + 2: 14.0 KB at
// r = 6, 50.6 KB at r = 32 - three workgroups per CU at the largest radius.  Every global read is bounds-checked against the grid, and
// the integer part of the shift is clamped before it is converted, so no input value moves a read outside the tensors.
#include "track_blur.h"

namespace ccvpe {

__global__ __launch_bounds__(256) void track_predict_kernel(const TrackPredictParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tp_smem[];
    constexpr int HW = TAIL_HW, n = HW * HW;
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const int r = p.radius, S = track_side(r), P = track_pitch(r), WL = track_wlen(r);
    const int Y0 = (t / (HW / TRACK_T)) * TRACK_T, X0 = (t % (HW / TRACK_T)) * TRACK_T;
    float* mid = reinterpret_cast<float*>(tp_smem);   // [S][32] x-pass result (16-byte aligned rows)
    float* wx = mid + S * TRACK_T;                      // [WL] merged weights along x, wx[3 + k] = u[k]
    float* wy = wx + WL;                             // [WL] along y
    float* src = wy + WL;                            // [S][P] staged source
    const float dx = p.shift[b * 2 + 0], dy = p.shift[b * 2 + 1];
    const float fdx = floorf(dx), fdy = floorf(dy);
    // integer part clamped to +-2048 (beyond +-544 nothing of the grid is left in reach; NaN clamps to -2048): the conversion is defined
    const int ix = (int)fminf(fmaxf(fdx, -2048.f), 2048.f), iy = (int)fminf(fmaxf(fdy, -2048.f), 2048.f);
    const float fx = dx - fdx, fy = dy - fdy;         // exact for finite shifts, in [0, 1)
    const float* taps = p.taps + (size_t)b * p.taps_stride;
    if (tid < 2 * WL) {
        const bool y = tid >= WL;
        const int k = (y ? tid - WL : tid) - 3;
        const float f = y ? fy : fx;
        float u = 0.f;
        if (k >= 0 && k <= 2 * r + 1) {
            const int a = k - r < 0 ? r - k : k - r, c = k - 1 - r < 0 ? r + 1 - k : k - 1 - r;   // |k - r|, |k - 1 - r|
            const float ta = a <= r ? taps[a] : 0.f, tc = c <= r ? taps[c] : 0.f;
            u = fmaf(f, ta, (1.f - f) * tc);
        }
        (y ? wy : wx)[k + 3] = u;
    }
    // source rows gy0 .. gy0 + S - 1, columns gx0 .. gx0 + S - 1: a wave per row, lanes along the row
    const float* bel = p.belief + (size_t)b * n;
    const int gx0 = X0 - ix - r - 1, gy0 = Y0 - iy - r - 1;
    const int lane = tid & 63, wave = tid >> 6;
    for (int ly = wave; ly < S; ly += 4) {
        const int gy = gy0 + ly;
        const bool rowin = (unsigned)gy < (unsigned)HW;
        for (int lx = lane; lx < S; lx += 64) {
            const int gx = gx0 + lx;
            src[ly * P + lx] = rowin && (unsigned)gx < (unsigned)HW ? bel[gy * HW + gx] : 0.f;
        }
    }
    __syncthreads();
    track_blur_store<1>(src, S, P, mid, wx, wy, r, p.floor, p.log_prior, b, Y0, X0);
}

void launch_track_predict(const TrackPredictParams& p, hipStream_t s) {
    const size_t lds = track_lds_bytes(p.radius);
    static LdsAttr attr;
    ensure_dynamic_lds(attr, reinterpret_cast<const void*>(track_predict_kernel), lds);
    CCVPE_LAUNCH(track_predict_kernel, dim3(TRACK_TILES, p.B), dim3(256), lds, s, p);
}

}  // namespace ccvpe
