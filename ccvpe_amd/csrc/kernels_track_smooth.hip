// Backward pass over stored beliefs (ccvpe_track_smooth): the smoothing half of the histogram filter over the 512 x 512
// output grid.  Per query, with b the filter posterior of frame t, s' the smoothed map of frame t + 1 and (dx, dy), taps, floor the
// arguments of the ccvpe_track_predict call that carried b into frame t + 1 (P(m; d) = that call's c for a map m):
//
//     prior = P(b; dx, dy) + floor                      the bits track_predict_kernel takes the logf of
//     g     = s' > 0 ? s' / prior : 0                   NaN and negative s' are not taken
//     G     = sum g
//     a     = fmaf(floor, G, P(g; -dx, -dy))            P with the negated shift is the adjoint of P (symmetric taps, tent weights)
//     w     = b * a,  Z = sum w,  s = w * (1 / Z)
//
// Three launches, each grid-wide sum between two of them:
//   track_smooth_ratio_kernel   (256 tiles, B)  predict's staging of b and its two passes; g stored to `work`, the tile's sum of g
//   track_smooth_weight_kernel  (256 tiles, B)  the same staging on g with the negated shift; G from the 256 tile sums; w stored to
//                                               `smoothed` (G == 0: b itself); the tile's sum of w and its (max, first index)
//   track_smooth_scale_kernel   (64 chunks, B)  Z and the argmax from the 256 tile partials; the map scaled in place; stats
// The two blur kernels run track_blur.h's passes out of track_predict_kernel's LDS layout (50.6 KB at r = 32, plus 64 bytes for the
// reductions).  Every sum has one order - a thread's four values left to right, xor shuffles over the wave, waves 0 .. 3 in turn; the
// 256 tile partials as lane l: ((p[l] + p[l + 64]) + p[l + 128]) + p[l + 192], then the xor shuffles - and nothing is accumulated
// with atomics, so the same inputs give the same bits, alone as in a batch.  No counters: the launch boundaries are the hand-offs.
// `smoothed` may be `smoothed_next`: s' is read by the first launch only, and every cell by the thread that later writes it.
#include "tail_shared.h"
#include "track_blur.h"
#include "track_smooth_work.h"

namespace ccvpe {

size_t track_smooth_work_bytes(int B) { return sizeof(float) * SMOOTH_WORK_FLOATS * (size_t)B; }

__global__ __launch_bounds__(256) void track_smooth_ratio_kernel(const TrackSmoothParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sr_smem[];
    __shared__ float red[4];
    constexpr int HW = TAIL_HW, n = HW * HW;
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const int r = p.radius;
    const int Y0 = (t / (HW / TRACK_T)) * TRACK_T, X0 = (t % (HW / TRACK_T)) * TRACK_T;
    const TrackTile tile = track_tile(sr_smem, r);
    const SmoothWork wk = smooth_work(p.work, b);
    track_stage_shifted(tile, p.belief, p.shift, 1.f, p.taps, p.taps_stride, b, r, Y0, X0);
    __syncthreads();
    const float4 c = track_blur_passes<1>(tile.src, tile.S, tile.P, tile.mid, tile.wx, tile.wy, r);
    const int cell = (Y0 + (tid >> 3)) * HW + X0 + (tid & 7) * 4;
    const float fl = p.floor[b];
    const float4 sn = *reinterpret_cast<const float4*>(p.next + (size_t)b * n + cell);
    float4 g;
    g.x = sn.x > 0.f ? sn.x / (c.x + fl) : 0.f;
    g.y = sn.y > 0.f ? sn.y / (c.y + fl) : 0.f;
    g.z = sn.z > 0.f ? sn.z / (c.z + fl) : 0.f;
    g.w = sn.w > 0.f ? sn.w / (c.w + fl) : 0.f;
    *reinterpret_cast<float4*>(wk.g + cell) = g;
    const float s = smooth_wave_sum(((g.x + g.y) + g.z) + g.w);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) wk.gsum[t] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void track_smooth_weight_kernel(const TrackSmoothParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sw_smem[];
    __shared__ float red[4], redv[4], redG;
    __shared__ int redi[4];
    constexpr int HW = TAIL_HW, n = HW * HW;
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const int r = p.radius;
    const int Y0 = (t / (HW / TRACK_T)) * TRACK_T, X0 = (t % (HW / TRACK_T)) * TRACK_T;
    const TrackTile tile = track_tile(sw_smem, r);
    const SmoothWork wk = smooth_work(p.work, b);
    if (tid < 64) {
        const float G = smooth_sum_tiles(wk.gsum);
        if (tid == 0) redG = G;
    }
    // g is one more [512][512] map: query b of a batch of maps that are SMOOTH_WORK_FLOATS apart is map 0 of the batch at wk.g
    track_stage_shifted(tile, wk.g, p.shift + b * 2, -1.f, p.taps + (size_t)b * p.taps_stride, 0, 0, r, Y0, X0);
    __syncthreads();
    const float4 c = track_blur_passes<1>(tile.src, tile.S, tile.P, tile.mid, tile.wx, tile.wy, r);
    const int cell = (Y0 + (tid >> 3)) * HW + X0 + (tid & 7) * 4;
    const float fl = p.floor[b], G = redG;
    const float4 bq = *reinterpret_cast<const float4*>(p.belief + (size_t)b * n + cell);
    float4 w;
    // G == 0: the next map has no positive cell and says nothing; the result is the belief itself
    w.x = G == 0.f ? bq.x : bq.x * fmaf(fl, G, c.x);
    w.y = G == 0.f ? bq.y : bq.y * fmaf(fl, G, c.y);
    w.z = G == 0.f ? bq.z : bq.z * fmaf(fl, G, c.z);
    w.w = G == 0.f ? bq.w : bq.w * fmaf(fl, G, c.w);
    *reinterpret_cast<float4*>(p.smoothed + (size_t)b * n + cell) = w;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    argmax_merge(best, bi, w.x, cell);
    argmax_merge(best, bi, w.y, cell + 1);
    argmax_merge(best, bi, w.z, cell + 2);
    argmax_merge(best, bi, w.w, cell + 3);
    argmax_wave(best, bi);
    const float s = smooth_wave_sum(((w.x + w.y) + w.z) + w.w);
    if ((tid & 63) == 0) { red[tid >> 6] = s; redv[tid >> 6] = best; redi[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < 4; ++v) argmax_merge(best, bi, redv[v], redi[v]);
        wk.wsum[t] = ((red[0] + red[1]) + red[2]) + red[3];
        wk.wmax[t] = best;
        wk.widx[t] = __int_as_float(bi);
    }
}

static constexpr int SMOOTH_CHUNKS = 64;   // of 4096 cells: four float4 per thread

__global__ __launch_bounds__(256) void track_smooth_scale_kernel(const TrackSmoothParams p) {
    __shared__ float sh[4];   // G, Z, the largest w, its first index (int bits)
    constexpr int n = TAIL_HW * TAIL_HW;
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const SmoothWork wk = smooth_work(p.work, b);
    if (tid < 64) {
        const float G = smooth_sum_tiles(wk.gsum), Z = smooth_sum_tiles(wk.wsum);
        float best = -INFINITY;
        int bi = 0x7fffffff;
        for (int v = 0; v < 4; ++v) argmax_merge(best, bi, wk.wmax[tid + v * 64], __float_as_int(wk.widx[tid + v * 64]));
        argmax_wave(best, bi);
        if (tid == 0) { sh[0] = G; sh[1] = Z; sh[2] = best; sh[3] = __int_as_float(bi); }
    }
    __syncthreads();
    const float G = sh[0], Z = sh[1], best = sh[2];
    const int bi = __float_as_int(sh[3]);
    const bool keep = G == 0.f;                        // the map already holds b
    const bool good = isfinite(Z) && Z > 0.f;
    const float inv = 1.f / Z;
    if (!keep) {
        float4* m = reinterpret_cast<float4*>(p.smoothed + (size_t)b * n + (size_t)chunk * (n / SMOOTH_CHUNKS));
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = m[tid + u * 256];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            m[tid + u * 256] = good ? make_float4(v[u].x * inv, v[u].y * inv, v[u].z * inv, v[u].w * inv) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (chunk == 0 && tid == 0) {
        // a value is taken when it is above -inf; a map without one has no argmax
        const bool taken = best > -INFINITY && (unsigned)bi < (unsigned)n;
        float* st = p.stats + (size_t)b * 4;
        if (keep) {
            st[0] = taken ? (float)bi : -1.f; st[1] = taken ? best : NAN; st[2] = NAN; st[3] = G;
        } else if (good && taken) {
            st[0] = (float)bi; st[1] = best * inv; st[2] = Z; st[3] = G;
        } else {
            st[0] = -1.f; st[1] = NAN; st[2] = Z; st[3] = G;
        }
    }
}

void launch_track_smooth(const TrackSmoothParams& p, hipStream_t s) {
    const size_t lds = track_lds_bytes(p.radius);
    static LdsAttr weight_attr;
    ensure_dynamic_lds(weight_attr, reinterpret_cast<const void*>(track_smooth_weight_kernel), lds);
    launch_track_smooth_ratio(p, s);
    CCVPE_LAUNCH(track_smooth_weight_kernel, dim3(TRACK_TILES, p.B), dim3(256), lds, s, p);
    launch_track_smooth_scale(p, s);
}

// the first launch alone: the link statistics (kernels_track_link.hip) start with it, so their g and G are the smoother's bits
void launch_track_smooth_ratio(const TrackSmoothParams& p, hipStream_t s) {
    const size_t lds = track_lds_bytes(p.radius);
    static LdsAttr ratio_attr;
    ensure_dynamic_lds(ratio_attr, reinterpret_cast<const void*>(track_smooth_ratio_kernel), lds);
    CCVPE_LAUNCH(track_smooth_ratio_kernel, dim3(TRACK_TILES, p.B), dim3(256), lds, s, p);
}

// the last launch alone: the affine smoother (kernels_track_smooth_affine.hip) ends with it, on the same work layout
void launch_track_smooth_scale(const TrackSmoothParams& p, hipStream_t s) {
    CCVPE_LAUNCH(track_smooth_scale_kernel, dim3(SMOOTH_CHUNKS, p.B), dim3(256), 0, s, p);
}

}  // namespace ccvpe
