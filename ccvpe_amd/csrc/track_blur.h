// The blur passes and the log store track_predict_kernel (kernels_track.hip) and track_predict_affine_kernel (kernels_track_affine.hip)
// share: one definition, so that the affine kernel at an integer translation gives track_predict_kernel's bits.  Each
// kernel stages its own source tile; the files that include this are built with -fno-slp-vectorize (ccvpe_amd/build.py).
#pragma once
#include "kernels.h"

namespace ccvpe {

static constexpr int TRACK_T = 32;                 // tile side
static constexpr int TRACK_TILES = (TAIL_HW / TRACK_T) * (TAIL_HW / TRACK_T);   // 256 per query: one per CU at batch 1

// A workgroup of 256 threads behind the barrier that completed its staged source src [S][P] (row pitch P) and the weights of a pass,
// wx[3 + k] and wy[3 + k], k = 0 .. 2r + MERGED, zero-padded by 3 on both sides for the x pass' four outputs per thread: the 2r + 1
// taps of the blur, or with MERGED = 1 the 2r + 2 of the blur merged with a 2-tap shift.  x pass out of src into mid [S][32] (16-byte
// aligned rows), y pass out of that, logf(blur + floor[b]) as one float4 per thread into the tile at (X0, Y0) of log_prior[b].  A pass
// is that many fused multiply-adds per output in ascending source index from a zero accumulator.
template <int MERGED>
__device__ __forceinline__ void track_blur_store(const float* src, int S, int P, float* mid, const float* wx, const float* wy, int r,
                                                 const float* floor, float* log_prior, int b, int Y0, int X0) {
    constexpr int HW = TAIL_HW, n = HW * HW;
    const int tid = threadIdx.x;
    // x pass: task = (row, 4 adjacent columns); source column x4 + c feeds output i with weight wx[3 + c - i]
    for (int i = tid; i < S * (TRACK_T / 4); i += 256) {
        const int ly = i >> 3, x4 = (i & 7) * 4;
        const float* row = src + ly * P + x4;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        float w1 = 0.f, w2 = 0.f, w3 = 0.f;          // the weights of outputs 1 .. 3 for this column: wx[3 + c - 1], [.. - 2], [.. - 3]
        for (int c = 0; c <= 2 * r + MERGED + 3; ++c) {
            const float v = row[c], w0 = wx[3 + c];
            a0 = fmaf(w0, v, a0); a1 = fmaf(w1, v, a1); a2 = fmaf(w2, v, a2); a3 = fmaf(w3, v, a3);
            w3 = w2; w2 = w1; w1 = w0;
        }
        *reinterpret_cast<float4*>(mid + ly * TRACK_T + x4) = make_float4(a0, a1, a2, a3);
    }
    __syncthreads();
    // y pass: thread = (output row, 4 adjacent columns)
    const int y = tid >> 3, x4 = (tid & 7) * 4;
    const float4* col = reinterpret_cast<const float4*>(mid + y * TRACK_T + x4);
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k <= 2 * r + MERGED; ++k) {
        const float4 v = col[k * (TRACK_T / 4)];
        const float w = wy[3 + k];
        a.x = fmaf(w, v.x, a.x); a.y = fmaf(w, v.y, a.y); a.z = fmaf(w, v.z, a.z); a.w = fmaf(w, v.w, a.w);
    }
    const float fl = floor[b];
    float4* dst = reinterpret_cast<float4*>(log_prior + (size_t)b * n + (size_t)(Y0 + y) * HW + X0 + x4);
    *dst = make_float4(logf(a.x + fl), logf(a.y + fl), logf(a.z + fl), logf(a.w + fl));
}

}  // namespace ccvpe
