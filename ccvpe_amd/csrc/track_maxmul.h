// The max-product passes of the MAP trajectory (kernels_track_viterbi.hip): track_blur.h's two passes with the sum
// replaced by a maximum, out of the same LDS layout and in the same thread mapping, and the merged weights of one cell's window for the
// backtrack.  A pass has no sum of its own: every candidate is one float32 product, and the maximum is exact, so the order of the
// candidates does not matter.  A candidate enters as `c > acc ? c : acc` from acc = 0: NaN and negative products never do.
#pragma once
#include "track_blur.h"

namespace ccvpe {

__device__ __forceinline__ float maxmul_take(float acc, float c) { return c > acc ? c : acc; }

// What the step kernels of the two motion models share (kernels_track_viterbi.hip, kernels_track_viterbi_affine.hip): the hand-off to
// track_viterbi_scale_kernel, the guarded previous index and the cleaned product.
static constexpr int VITERBI_WORK_FLOATS = 2 * TRACK_TILES;   // per query: the tiles' largest w [256], its first index [256] (int bits)

// j = (int) prev_stats[0] when that is a cell index, else -1 (NaN fails both comparisons)
__device__ __forceinline__ int viterbi_prev_index(const float* prev_stats, int b) {
    const float s = prev_stats[(size_t)b * 4];
    return s >= 0.f && s < (float)(TAIL_HW * TAIL_HW) ? (int)s : -1;
}
__device__ __forceinline__ float viterbi_clean(float w) { return w > 0.f ? w : 0.f; }

// A workgroup of 256 threads behind the barrier that completed its staged source (src [S][P], wx[3 + k], wy[3 + k], k = 0 .. 2r + MERGED,
// zero-padded by 3 on both sides): thread tid gets, for row tid >> 3, columns (tid & 7) * 4 .. + 3 of the tile,
//     max over ky of fl(wy[ky] * max over kx of fl(wx[kx] * src))
// x pass out of src into mid [S][32], y pass out of that, as track_blur_tile<MERGED> walks them: MERGED = 1 behind track_stage_shifted
// (2r + 2 merged weights), MERGED = 0 behind the affine sampling (the 2r + 1 symmetric taps, kernels_track_viterbi_affine.hip).
template <int MERGED>
__device__ __forceinline__ float4 track_maxmul_passes(const float* src, int S, int P, float* mid, const float* wx, const float* wy, int r) {
    const int tid = threadIdx.x;
    // x pass: task = (row, 4 adjacent columns); source column x4 + c is candidate c - i of output i, with weight wx[3 + c - i]
    for (int i = tid; i < S * (TRACK_T / 4); i += 256) {
        const int ly = i >> 3, x4 = (i & 7) * 4;
        const float* row = src + ly * P + x4;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        float w1 = 0.f, w2 = 0.f, w3 = 0.f;
        for (int c = 0; c <= 2 * r + MERGED + 3; ++c) {
            const float v = row[c], w0 = wx[3 + c];
            a0 = maxmul_take(a0, w0 * v); a1 = maxmul_take(a1, w1 * v); a2 = maxmul_take(a2, w2 * v); a3 = maxmul_take(a3, w3 * v);
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
        a.x = maxmul_take(a.x, w * v.x); a.y = maxmul_take(a.y, w * v.y); a.z = maxmul_take(a.z, w * v.z); a.w = maxmul_take(a.w, w * v.w);
    }
    return a;
}

// One axis of a shift as track_stage_shifted splits it: the integer part, clamped to +-2048 before it is converted (NaN clamps to
// -2048), and the fraction in [0, 1)
struct ShiftAxis { int i; float f; };
__device__ __forceinline__ ShiftAxis track_shift_axis(float d) {
    const float fd = floorf(d);
    ShiftAxis a;
    a.i = (int)fminf(fmaxf(fd, -2048.f), 2048.f);
    a.f = d - fd;
    return a;
}
// Merged weight k = 0 .. 2r + 1 of a pass, track_stage_shifted's expression: it belongs to source index x' - i - r - 1 + k
__device__ __forceinline__ float track_merged_weight(const float* taps, int r, float f, int k) {
    const int a = k - r < 0 ? r - k : k - r, c = k - 1 - r < 0 ? r + 1 - k : k - 1 - r;   // |k - r|, |k - 1 - r|
    const float ta = a <= r ? taps[a] : 0.f, tc = c <= r ? taps[c] : 0.f;
    return fmaf(f, ta, (1.f - f) * tc);
}

}  // namespace ccvpe
