// The hand-off buffer and the sums the smoother's kernels share (kernels_track_smooth.hip; kernels_track_smooth_affine.hip,
// DESIGN.md 4.22): one layout of `work`, so that track_smooth_scale_kernel ends both, and one order of every sum.
#pragma once
#include "tail_shared.h"
#include "track_blur.h"

namespace ccvpe {

// floats of `work` per query: the g map, then the tiles' sums of g, sums of w, maxima of w and (as bits) their first indices
static constexpr size_t SMOOTH_WORK_FLOATS = (size_t)TAIL_HW * TAIL_HW + 4 * TRACK_TILES;

struct SmoothWork {
    float* g;       // [512*512]
    float* gsum;    // [256]
    float* wsum;    // [256]
    float* wmax;    // [256]
    float* widx;    // [256] int bits
};
__device__ __forceinline__ SmoothWork smooth_work(float* work, int b) {
    constexpr int n = TAIL_HW * TAIL_HW;
    SmoothWork w;
    w.g = work + (size_t)b * SMOOTH_WORK_FLOATS;
    w.gsum = w.g + n;
    w.wsum = w.gsum + TRACK_TILES;
    w.wmax = w.wsum + TRACK_TILES;
    w.widx = w.wmax + TRACK_TILES;
    return w;
}

// every thread's value -> the wave's sum in all of its lanes
__device__ __forceinline__ float smooth_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
// the first wave: the sum of a query's 256 tile partials, in all of its lanes
__device__ __forceinline__ float smooth_sum_tiles(const float* part) {
    const int l = threadIdx.x & 63;
    return smooth_wave_sum(((part[l] + part[l + 64]) + part[l + 128]) + part[l + 192]);
}

}  // namespace ccvpe
