// Link statistics of a smoothed stream (ccvpe_track_link): the pairwise posterior p(x_t, x_t+1 | frames 1..T) of one link of
// a stream of ccvpe_track_predict calls, binned by displacement - the expected transition counts a motion model is fitted to.  Per query,
// with b the filter posterior of frame t, s' the smoothed map of frame t + 1 and (dx, dy), taps, floor the arguments of the predict call
// between them (i = floor(d) clamped to +-2048, f = d - floor(d) per axis, u[k] = fmaf(f, t[|k - r|], (1.f - f) * t[|k - 1 - r|]),
// k = 0 .. 2r + 1, K = 2r + 2):
//
//     prior, g, G    ccvpe_track_smooth's, the bits of its first launch
//     Sb             = sum b
//     D[ky][kx]      = sum over target cells (y', x') of g(y', x') * b(y' - iy - r - 1 + ky, x' - ix - r - 1 + kx)      b zero-extended
//     moves[ky][kx]  = (uy[ky] * ux[kx]) * D[ky][kx]
//     M = sum moves,  J = (floor * G) * Sb,  Z = M + J,  stats = (Z, G, J, M)
//
// Four launches, each grid-wide sum between two of them:
//   track_smooth_ratio_kernel  (256 tiles, B)          kernels_track_smooth.hip's, unchanged: g and the tiles' sums of g, in SmoothWork
//   track_link_corr_kernel     (256 tiles, B)          predict's staging of b; the tile's K * K sums and its sum of b, to `work`
//   track_link_moves_kernel    (ceil(K K / 256), B)    per offset the 256 tile sums, the weight; moves stored
//   track_link_stats_kernel    (B)                     M from moves, G and Sb from the tile sums; stats
// The orders of the sums.  A tile's D[ky][kx]: thread (ty = tid & 31, q = tid >> 5) holds row ty of the tile's g in registers and makes, for
// the offsets kx = 4 kg .. 4 kg + 3 of its groups kg = q, q + 8, .., the row's sum as 32 fused multiply-adds in ascending tx from a zero
// accumulator, out of one sliding read of 35 cells of source row ty + ky; the 32 rows of a half wave are then added by xor shuffles over
// 16, 8, 4, 2, 1.  An offset's 256 tile sums: four chains over the tiles j, j + 4, .. (j = 0 .. 3), each in ascending order, then
// ((a0 + a1) + a2) + a3.  M: thread i adds moves[i], moves[i + 256], .. in ascending order, then the wave's xor shuffles, waves 0 .. 3 in
// turn.  Sb: a thread's four cells left to right, the wave's xor shuffles, waves 0 .. 3 in turn; its and G's 256 tile sums in
// smooth_sum_tiles' order.  Nothing is accumulated with atomics, so the same inputs give the same bits, alone as in a batch.
#include "tail_shared.h"
#include "track_blur.h"
#include "track_smooth_work.h"

namespace ccvpe {

// `work`: SmoothWork of every query (the ratio launch addresses it by query; wsum holds the tiles' sums of b here, wmax and widx are not
// used), then per query the tiles' partial sums [256][K][K]
__host__ __device__ constexpr size_t link_part_floats(int r) { return (size_t)TRACK_TILES * (2 * r + 2) * (2 * r + 2); }
size_t track_link_work_bytes(int B, int r) { return sizeof(float) * (SMOOTH_WORK_FLOATS + link_part_floats(r)) * (size_t)B; }
__device__ __forceinline__ float* link_part(float* work, int B, int b, int r) {
    return work + (size_t)B * SMOOTH_WORK_FLOATS + (size_t)b * link_part_floats(r);
}

// The sliding read runs up to two cells past the end of a source row for the offsets kx = K, K + 1 of a last group, which are not stored:
// behind the last row of the staged source that is past track_lds_bytes(r)
static constexpr size_t LINK_LDS_PAD = 16;

__global__ __launch_bounds__(256) void track_link_corr_kernel(const TrackLinkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lc_smem[];
    __shared__ float red[4];
    constexpr int HW = TAIL_HW, n = HW * HW;
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const int r = p.radius, K = 2 * r + 2;
    const int Y0 = (t / (HW / TRACK_T)) * TRACK_T, X0 = (t % (HW / TRACK_T)) * TRACK_T;
    const TrackTile tile = track_tile(lc_smem, r);
    const SmoothWork wk = smooth_work(p.work, b);
    track_stage_shifted(tile, p.belief, p.shift, 1.f, p.taps, p.taps_stride, b, r, Y0, X0);
    // the tile's own cells of b
    const float4 bq = *reinterpret_cast<const float4*>(p.belief + (size_t)b * n + (Y0 + (tid >> 3)) * HW + X0 + (tid & 7) * 4);
    const float s = smooth_wave_sum(((bq.x + bq.y) + bq.z) + bq.w);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    // row ty of the tile's g
    const int ty = tid & 31, q = tid >> 5;
    float gr[TRACK_T];
    const float4* grow = reinterpret_cast<const float4*>(wk.g + (Y0 + ty) * HW + X0);
#pragma unroll
    for (int i = 0; i < TRACK_T / 4; ++i) {
        const float4 v = grow[i];
        gr[4 * i] = v.x; gr[4 * i + 1] = v.y; gr[4 * i + 2] = v.z; gr[4 * i + 3] = v.w;
    }
    __syncthreads();
    if (tid == 0) wk.wsum[t] = ((red[0] + red[1]) + red[2]) + red[3];
    float* part = link_part(p.work, p.B, b, r) + (size_t)t * (K * K);
    const int groups = (K + 3) >> 2;
    for (int ky = 0; ky < K; ++ky) {
        for (int kg = q; kg < groups; kg += 8) {
            // source column 4 kg + c of row ty + ky meets g column c - i at offset kx = 4 kg + i
            const float* src = tile.src + (ty + ky) * tile.P + 4 * kg;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
            for (int c = 0; c < TRACK_T + 3; ++c) {
                const float v = src[c];
                if (c < TRACK_T) a0 = fmaf(gr[c < TRACK_T ? c : 0], v, a0);
                if (c >= 1 && c < TRACK_T + 1) a1 = fmaf(gr[c >= 1 && c < TRACK_T + 1 ? c - 1 : 0], v, a1);
                if (c >= 2 && c < TRACK_T + 2) a2 = fmaf(gr[c >= 2 && c < TRACK_T + 2 ? c - 2 : 0], v, a2);
                if (c >= 3) a3 = fmaf(gr[c >= 3 ? c - 3 : 0], v, a3);
            }
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) {
                a0 += __shfl_xor(a0, off); a1 += __shfl_xor(a1, off); a2 += __shfl_xor(a2, off); a3 += __shfl_xor(a3, off);
            }
            if (ty == 0) {
                float* d = part + ky * K + 4 * kg;
                d[0] = a0; d[1] = a1;                       // K is even: a group holds four offsets or two
                if (4 * kg + 2 < K) { d[2] = a2; d[3] = a3; }
            }
        }
    }
}

// u[k] of one axis: the statement of track_stage_shifted
__device__ __forceinline__ float link_weight(const float* taps, float d, int k, int r) {
    const float f = d - floorf(d);
    const int a = k - r < 0 ? r - k : k - r, c = k - 1 - r < 0 ? r + 1 - k : k - 1 - r;
    const float ta = a <= r ? taps[a] : 0.f, tc = c <= r ? taps[c] : 0.f;
    return fmaf(f, ta, (1.f - f) * tc);
}

__global__ __launch_bounds__(256) void track_link_moves_kernel(const TrackLinkParams p) {
    const int b = blockIdx.y, r = p.radius, K = 2 * r + 2, KK = K * K;
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= KK) return;
    const float* part = link_part(p.work, p.B, b, r) + o;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int t = 0; t < TRACK_TILES; t += 4) {
        a0 += part[(size_t)t * KK]; a1 += part[(size_t)(t + 1) * KK]; a2 += part[(size_t)(t + 2) * KK]; a3 += part[(size_t)(t + 3) * KK];
    }
    const float D = ((a0 + a1) + a2) + a3;
    const float* taps = p.taps + (size_t)b * p.taps_stride;
    const float ux = link_weight(taps, p.shift[b * 2 + 0], o % K, r), uy = link_weight(taps, p.shift[b * 2 + 1], o / K, r);
    p.moves[(size_t)b * KK + o] = (uy * ux) * D;
}

__global__ __launch_bounds__(256) void track_link_stats_kernel(const TrackLinkParams p) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x, r = p.radius, KK = (2 * r + 2) * (2 * r + 2);
    const SmoothWork wk = smooth_work(p.work, b);
    const float* mv = p.moves + (size_t)b * KK;
    float m = 0.f;
    for (int i = tid; i < KK; i += 256) m += mv[i];
    m = smooth_wave_sum(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid < 64) {
        const float G = smooth_sum_tiles(wk.gsum), Sb = smooth_sum_tiles(wk.wsum);
        if (tid == 0) {
            const float M = ((red[0] + red[1]) + red[2]) + red[3];
            const float J = (p.floor[b] * G) * Sb;
            float* st = p.stats + (size_t)b * 4;
            st[0] = M + J; st[1] = G; st[2] = J; st[3] = M;
        }
    }
}

void launch_track_link(const TrackLinkParams& p, hipStream_t s) {
    TrackSmoothParams q{};
    q.belief = p.belief; q.next = p.next; q.shift = p.shift; q.taps = p.taps; q.taps_stride = p.taps_stride; q.radius = p.radius;
    q.floor = p.floor; q.work = p.work; q.B = p.B;
    launch_track_smooth_ratio(q, s);
    const size_t lds = track_lds_bytes(p.radius) + LINK_LDS_PAD;
    const int KK = (2 * p.radius + 2) * (2 * p.radius + 2);
    static LdsAttr corr_attr;
    ensure_dynamic_lds(corr_attr, reinterpret_cast<const void*>(track_link_corr_kernel), lds);
    CCVPE_LAUNCH(track_link_corr_kernel, dim3(TRACK_TILES, p.B), dim3(256), lds, s, p);
    CCVPE_LAUNCH(track_link_moves_kernel, dim3((KK + 255) / 256, p.B), dim3(256), 0, s, p);
    CCVPE_LAUNCH(track_link_stats_kernel, dim3(p.B), dim3(256), 0, s, p);
}

}  // namespace ccvpe
