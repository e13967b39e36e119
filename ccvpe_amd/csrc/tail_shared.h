// Device helpers the output-side kernels share across files (kernels_tail.hip, kernels_heading.hip, kernels_hprior.hip): the softmax
// statistics of a sample from its chunk partials, the fixed-order float64 reduction of the posterior summary - thread
// -> xor shuffles -> four waves in LDS - and the heading bin of a field cell.  One definition, so the same order of operations and the
// same bits wherever they are used.
#pragma once
#include "kernels.h"
#include "ticket.h"

namespace ccvpe {

__device__ __forceinline__ void combine(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    if (mn == -INFINITY) { s = 0.f; return; }   // both sides empty: exp(-inf - -inf) would be NaN
    s = s * __expf(m - mn) + s2 * __expf(m2 - mn);
    m = mn;
}

// the sample's (max, 1 / sum) from its chunk partials, into LDS (gm, gs); the caller meets at a barrier before reading them.  Shared by
// softmax_final_kernel, pose_argmax_kernel and heading_reduce_kernel: the same order of combines, so the same bits
__device__ __forceinline__ void softmax_stats(const float* partial, int b, int chunks, float& gm, float& gs) {
    if (threadIdx.x < 64) {
        float m = -INFINITY, s = 0.f;
        for (int i = threadIdx.x; i < chunks; i += 64)
            combine(m, s, partial[((size_t)b * chunks + i) * 2], partial[((size_t)b * chunks + i) * 2 + 1]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float m2 = __shfl_xor(m, off), s2 = __shfl_xor(s, off);
            combine(m, s, m2, s2);
        }
        if (threadIdx.x == 0) { gm = m; gs = 1.f / s; }
    }
}

// The heading of a cell of the orientation field, shared by heading_reduce_kernel and heading_prior_map_kernel: a cell
// has a heading when c and s are finite and not both zero ...
__device__ __forceinline__ bool heading_valid(float c, float s) { return isfinite(c) && isfinite(s) && !(c == 0.f && s == 0.f); }
// ... and its bin of nb (scale = (float)nb / 360.f): a result >= nb wraps, the rest is clamped to [0, nb)
__device__ __forceinline__ int heading_bin(float c, float s, float scale, int nb) {
    int bin = (int)(pose_angle_deg(c, s) * scale);
    if (bin >= nb) bin -= nb;
    return min(max(bin, 0), nb - 1);
}

// every thread: its sums -> the wave's (all lanes), lane 0 of each wave -> lds[wave][n]; the caller meets at a barrier, then ...
template <int n>
__device__ __forceinline__ void summ_wave_to_lds(double (&a)[n], double* lds) {
#pragma unroll
    for (int k = 0; k < n; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a[k] += __shfl_xor(a[k], off);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < n; ++k) lds[(threadIdx.x >> 6) * n + k] = a[k];
    }
}
// ... thread 0: the workgroup's sums, waves in order
template <int n>
__device__ __forceinline__ void summ_from_lds(double (&a)[n], const double* lds) {
#pragma unroll
    for (int w = 1; w < 4; ++w) {
#pragma unroll
        for (int k = 0; k < n; ++k) a[k] += lds[w * n + k];
    }
}

}  // namespace ccvpe
