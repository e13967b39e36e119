// Device helpers the output-side kernels share (kernels_tail.hip, kernels_heading.hip, kernels_hprior.hip): the softmax statistics of a
// sample from its chunk partials, the posterior's value at a cell, a chunk's loads, the (value, first index) argmax from thread to
// sample, the clipped window around the argmax, the fixed-order float64 reduction of the posterior summary - thread
// -> xor shuffles -> four waves in LDS -> lane = chunk - and the heading bin of a field cell.  One definition each, so the same order
// of operations and the same bits wherever they are used; tests/test_cabi.py keeps the two expressions the forms' bit-identity rests
// on, the tie-break and the posterior, out of every other file.
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

// The posterior at a cell: the expression softmax_final_kernel stores, for x = the logit (plus the prior, added first) and softmax_stats'
// (m, inv).  Every kernel that recomputes a value of the map calls this, so the recomputed bits are the stored ones
__device__ __forceinline__ float posterior_value(float x, float m, float inv) { return __expf(x - m) * inv; }

// Chunk `lo` of a sample as pose_argmax_kernel and heading_reduce_kernel read it: four float4 of logits per thread in one trip, with
// PRIOR four of the prior beside them and v = fl32(logit + prior)
template <bool PRIOR>
__device__ __forceinline__ void load_chunk(const float* logits, const float* prior, int lo, float4 (&v)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = reinterpret_cast<const float4*>(logits + lo)[threadIdx.x + u * 256];
    if constexpr (PRIOR) {
        float4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = reinterpret_cast<const float4*>(prior + lo)[threadIdx.x + u * 256];
#pragma unroll
        for (int u = 0; u < 4; ++u) { v[u].x += q[u].x; v[u].y += q[u].y; v[u].z += q[u].z; v[u].w += q[u].w; }
    }
}

// (value, first index) argmax: the larger value wins, the lower index on equal values; NaN never wins (both comparisons are false)
__device__ __forceinline__ void argmax_merge(float& best, int& bi, float v2, int i2) {
    if (v2 > best || (v2 == best && i2 < bi)) { best = v2; bi = i2; }
}
// ... over the wave, every lane
__device__ __forceinline__ void argmax_wave(float& best, int& bi) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float v2 = __shfl_xor(best, off);
        const int i2 = __shfl_xor(bi, off);
        argmax_merge(best, bi, v2, i2);
    }
}
// ... over the workgroup, from the waves' pairs: lane 0 of each wave -> sv, si [4]; a barrier (which the caller's own LDS hand-offs may
// share); thread 0 merges waves 1 .. 3 in order and hands the chunk's pair to the sample's last arriver (before ticket_arrive)
__device__ __forceinline__ void argmax_publish(float& best, int& bi, float* sv, int* si, float* pair) {
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = best; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) argmax_merge(best, bi, sv[w], si[w]);
        st_sc1(pair, best);
        st_sc1(pair + 1, __int_as_float(bi));
    }
}
// ... over the sample, by the first wave of its last arriver (behind ticket_arrive): lane = chunk loads its pair, then the wave.
// There are TAIL_CHUNKS = 64 chunks and 64 lanes, so a lane has exactly one pair and needs no seed.  The forms this replaces seeded a
// lane and merged its one pair into the seed: postprocess_kernel with (-inf, 0x7fffffff), pose_argmax_kernel with a first merge that
// always took the pair (the load, spelled as a merge).  Merging a pair (v, i) into (-inf, 0x7fffffff) gives (v, i) unless v is NaN or
// (v, i) is the seed itself: a chunk's v is never NaN (a thread starts at -inf and takes only values that compare greater; merges take
// only values that compare greater or equal), and a chunk of postprocess_kernel that took nothing publishes exactly (-inf, 0x7fffffff),
// the sentinel its "no posterior" rule tests.  So all three forms are the load.
__device__ __forceinline__ void argmax_from_pairs(const float* pairs, float& best, int& bi) {
    best = ld_sc1(pairs + threadIdx.x * 2);
    bi = __float_as_int(ld_sc1(pairs + threadIdx.x * 2 + 1));
    argmax_wave(best, bi);
}

// The clipped window |x - x*| <= r, |y - y*| <= r around cell bi of the map (summ_finish, heading_reduce_kernel): its cells in raster
// order, at(i, bi) the map index of cell i - past the window bi itself, a read inside the map whose value the caller adds as 0
struct Window {
    int x0, y0, ww, cells;
    __device__ __forceinline__ int at(int i, int bi) const {
        const int ly = i / ww;
        return i < cells ? (y0 + ly) * TAIL_HW + x0 + (i - ly * ww) : bi;
    }
};
__device__ __forceinline__ Window window_around(int bi, int r) {
    const int xs = bi & (TAIL_HW - 1), ys = (int)((unsigned)bi / TAIL_HW);   // (bi: a position of the map)
    const int x0 = max(xs - r, 0), x1 = min(xs + r, TAIL_HW - 1), y0 = max(ys - r, 0), y1 = min(ys + r, TAIL_HW - 1);
    const int ww = x1 - x0 + 1;
    return Window{x0, y0, ww, ww * (y1 - y0 + 1)};
}
static constexpr int WINDOW_UB = 6;   // window cells in flight per thread: r = 8 is one trip to memory, r = 32 three

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
// The first wave of a sample's last arriver (behind ticket_arrive): the sample's sums from its chunks' hand-off rows part[chunk][stride]
// (agent-scope stores of thread 0 of each chunk) - lane = chunk loads its row, then the xor shuffles; g is complete in lanes 0 .. 63
template <int n>
__device__ __forceinline__ void sums_from_chunks(const double* part, int stride, double (&g)[n]) {
    if (threadIdx.x < 64) {
#pragma unroll
        for (int k = 0; k < n; ++k) g[k] = ld_sc1(part + threadIdx.x * stride + k);
#pragma unroll
        for (int k = 0; k < n; ++k) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) g[k] += __shfl_xor(g[k], off);
        }
    }
}

}  // namespace ccvpe
