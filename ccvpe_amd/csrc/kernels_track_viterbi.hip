// MAP trajectory of a tracked stream (ccvpe_track_viterbi, ccvpe_track_viterbi_back): the max-product sweep over the
// stored beliefs of the histogram filter, with the filter's own mixture transition read as a latent choice per link - a move with the
// merged kernel u, or a jump with the relocalisation floor.  Per query, with b the filter posterior of frame t, b- that of frame
// t - 1, v- the score map of frame t - 1 and (dx, dy), taps, floor the arguments of the ccvpe_track_predict call between the two:
//
//     prior = P(b-; dx, dy) + floor                      the bits track_predict_kernel takes the logf of
//     lik   = b > 0 ? b / prior : 0                      the frame's likelihood up to a constant
//     win   = max_ky fl(uy[ky] * max_kx fl(ux[kx] * v-(source cell)))
//     m     = max(win, fl(floor * v-[j]))                j the first index of the largest v- (prev_stats[0])
//     w     = fl(lik * m), a w that is not > 0 stored as 0;   v = ldexpf(w, -e) with W = max w and W * 2^-e in [1, 2)
//
// Two launches per step and one per backtracked link:
//   track_viterbi_step_kernel   (256 tiles, B)  predict's staging of b- and its two blur passes, then the same LDS staged with v- and
//                                               the two max passes of track_maxmul.h; w stored to `score`, the tile's (max, first
//                                               index) to `work`.  The first frame (no b-) stores b itself; a restart (no j, or
//                                               v-[j] not > 0) stores lik and skips the second staging.
//   track_viterbi_scale_kernel  (64 chunks, B)  W and its first index from the 256 tile pairs; the map scaled in place by 2^-e, or
//                                               zeroed; stats
//   track_viterbi_back_kernel   (B)             the (2r + 2)^2 candidates of one cell straight from global memory
// The recursion has no sum of its own - the one blur is the smoother's prior - and the scaling is by a power of two, so the same
// inputs give the same bits, alone as in a batch.  No atomics, no counters: the launch boundary is the hand-off, through `work`.
#include "tail_shared.h"
#include "track_maxmul.h"

namespace ccvpe {

size_t track_viterbi_work_bytes(int B) { return sizeof(float) * VITERBI_WORK_FLOATS * (size_t)B; }

__global__ __launch_bounds__(256) void track_viterbi_step_kernel(const TrackViterbiParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char vs_smem[];
    __shared__ float redv[4];
    __shared__ int redi[4];
    constexpr int HW = TAIL_HW, n = HW * HW;
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const int Y0 = (t / (HW / TRACK_T)) * TRACK_T, X0 = (t % (HW / TRACK_T)) * TRACK_T;
    const int cell = (Y0 + (tid >> 3)) * HW + X0 + (tid & 7) * 4;
    float4 w = *reinterpret_cast<const float4*>(p.belief + (size_t)b * n + cell);
    if (p.belief_prev) {
        const int r = p.radius;
        const TrackTile tile = track_tile(vs_smem, r);
        track_stage_shifted(tile, p.belief_prev, p.shift, 1.f, p.taps, p.taps_stride, b, r, Y0, X0);
        __syncthreads();
        const float4 c = track_blur_passes<1>(tile.src, tile.S, tile.P, tile.mid, tile.wx, tile.wy, r);
        const float fl = p.floor[b];
        w.x = w.x > 0.f ? w.x / (c.x + fl) : 0.f;
        w.y = w.y > 0.f ? w.y / (c.y + fl) : 0.f;
        w.z = w.z > 0.f ? w.z / (c.z + fl) : 0.f;
        w.w = w.w > 0.f ? w.w / (c.w + fl) : 0.f;
        const int j = viterbi_prev_index(p.prev_stats, b);
        const float peak = j >= 0 ? p.score_prev[(size_t)b * n + j] : 0.f;
        if (peak > 0.f) {                       // the same for every thread of the query; else a restart: m = 1
            __syncthreads();                    // the y pass has read mid and wy
            track_stage_shifted(tile, p.score_prev, p.shift, 1.f, p.taps, p.taps_stride, b, r, Y0, X0);
            __syncthreads();
            const float4 win = track_maxmul_passes<1>(tile.src, tile.S, tile.P, tile.mid, tile.wx, tile.wy, r);
            const float jump = fl * peak;
            w.x = w.x * (jump > win.x ? jump : win.x);
            w.y = w.y * (jump > win.y ? jump : win.y);
            w.z = w.z * (jump > win.z ? jump : win.z);
            w.w = w.w * (jump > win.w ? jump : win.w);
        }
    }
    w = make_float4(viterbi_clean(w.x), viterbi_clean(w.y), viterbi_clean(w.z), viterbi_clean(w.w));
    *reinterpret_cast<float4*>(p.score + (size_t)b * n + cell) = w;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    argmax_merge(best, bi, w.x, cell);
    argmax_merge(best, bi, w.y, cell + 1);
    argmax_merge(best, bi, w.z, cell + 2);
    argmax_merge(best, bi, w.w, cell + 3);
    argmax_wave(best, bi);
    if ((tid & 63) == 0) { redv[tid >> 6] = best; redi[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < 4; ++v) argmax_merge(best, bi, redv[v], redi[v]);
        float* wk = p.work + (size_t)b * VITERBI_WORK_FLOATS;
        wk[t] = best;
        wk[TRACK_TILES + t] = __int_as_float(bi);
    }
}

static constexpr int VITERBI_CHUNKS = 64;   // of 4096 cells: four float4 per thread

__global__ __launch_bounds__(256) void track_viterbi_scale_kernel(const TrackViterbiParams p) {
    __shared__ float sh[2];   // the largest w, its first index (int bits)
    constexpr int n = TAIL_HW * TAIL_HW;
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const float* wk = p.work + (size_t)b * VITERBI_WORK_FLOATS;
    if (tid < 64) {
        float best = -INFINITY;
        int bi = 0x7fffffff;
        for (int v = 0; v < 4; ++v) argmax_merge(best, bi, wk[tid + v * 64], __float_as_int(wk[TRACK_TILES + tid + v * 64]));
        argmax_wave(best, bi);
        if (tid == 0) { sh[0] = best; sh[1] = __int_as_float(bi); }
    }
    __syncthreads();
    const float W = sh[0];
    const int bi = __float_as_int(sh[1]);
    const bool good = W > 0.f && isfinite(W) && (unsigned)bi < (unsigned)n;
    // e with W * 2^-e in [1, 2), from the bits: a subnormal W has its leading bit at 31 - clz
    const unsigned bits = __float_as_uint(W);
    const int ex = (int)((bits >> 23) & 0xff);
    const int e = ex ? ex - 127 : (31 - __clz((int)(bits & 0x7fffff))) - 149;
    float4* m = reinterpret_cast<float4*>(p.score + (size_t)b * n + (size_t)chunk * (n / VITERBI_CHUNKS));
    if (good) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = m[tid + u * 256];
#pragma unroll
        for (int u = 0; u < 4; ++u) m[tid + u * 256] = make_float4(ldexpf(v[u].x, -e), ldexpf(v[u].y, -e), ldexpf(v[u].z, -e), ldexpf(v[u].w, -e));
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) m[tid + u * 256] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (chunk == 0 && tid == 0) {
        bool restarted = true;
        if (p.belief_prev) {
            const int j = viterbi_prev_index(p.prev_stats, b);
            restarted = !((j >= 0 ? p.score_prev[(size_t)b * n + j] : 0.f) > 0.f);
        }
        float* st = p.stats + (size_t)b * 4;
        st[0] = good ? (float)bi : -1.f;
        st[1] = good ? ldexpf(W, -e) : NAN;
        st[2] = good ? (float)e : NAN;
        st[3] = restarted ? 1.f : 0.f;
    }
}

void launch_track_viterbi(const TrackViterbiParams& p, hipStream_t s) {
    const size_t lds = p.belief_prev ? track_lds_bytes(p.radius) : 0;
    static LdsAttr step_attr;
    ensure_dynamic_lds(step_attr, reinterpret_cast<const void*>(track_viterbi_step_kernel), lds);
    CCVPE_LAUNCH(track_viterbi_step_kernel, dim3(TRACK_TILES, p.B), dim3(256), lds, s, p);
    launch_track_viterbi_scale(p, s);
}

void launch_track_viterbi_scale(const TrackViterbiParams& p, hipStream_t s) {
    CCVPE_LAUNCH(track_viterbi_scale_kernel, dim3(VITERBI_CHUNKS, p.B), dim3(256), 0, s, p);
}

// One link of the backtrack: the source cell the path's `cell` of frame t came from, and the link's kind.  One workgroup per query;
// thread tid takes candidates tid, tid + 256, .. of the (2r + 2)^2 window in raster order.  Every read is guarded: j by
// viterbi_prev_index, cell against the grid, a candidate's source against the grid.
__global__ __launch_bounds__(256) void track_viterbi_back_kernel(const TrackViterbiBackParams p) {
    __shared__ float redv[4];
    __shared__ int redi[4];
    constexpr int HW = TAIL_HW, n = HW * HW;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int cell = p.cell[b];
    const int j = viterbi_prev_index(p.prev_stats, b);
    int* out = p.back + (size_t)b * 2;
    if ((unsigned)cell >= (unsigned)n || j < 0) {       // the end of a backtrack or the frame behind a broken one; no j: nothing to point at
        if (tid == 0) { out[0] = (unsigned)cell >= (unsigned)n ? j : -1; out[1] = VITERBI_LINK_START; }
        return;
    }
    const int r = p.radius, K = 2 * r + 2;
    const float* prev = p.score_prev + (size_t)b * n;
    const float* taps = p.taps + (size_t)b * p.taps_stride;
    const ShiftAxis ax = track_shift_axis(p.shift[b * 2 + 0]), ay = track_shift_axis(p.shift[b * 2 + 1]);
    const int gx0 = cell % HW - ax.i - r - 1, gy0 = cell / HW - ay.i - r - 1;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = tid; i < K * K; i += 256) {
        const int ky = i / K, kx = i - ky * K;
        const int gy = gy0 + ky, gx = gx0 + kx;
        if ((unsigned)gy < (unsigned)HW && (unsigned)gx < (unsigned)HW) {
            const float ux = track_merged_weight(taps, r, ax.f, kx), uy = track_merged_weight(taps, r, ay.f, ky);
            const float inner = ux * prev[gy * HW + gx];
            argmax_merge(best, bi, uy * inner, gy * HW + gx);
        }
    }
    argmax_wave(best, bi);
    if ((tid & 63) == 0) { redv[tid >> 6] = best; redi[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < 4; ++v) argmax_merge(best, bi, redv[v], redi[v]);
        const float jump = p.floor[b] * prev[j];
        if (!(best > 0.f) && !(jump > 0.f)) { out[0] = j; out[1] = VITERBI_LINK_START; }
        else if (jump > best) { out[0] = j; out[1] = VITERBI_LINK_JUMP; }
        else { out[0] = bi; out[1] = VITERBI_LINK_MOVE; }
    }
}

void launch_track_viterbi_back(const TrackViterbiBackParams& p, hipStream_t s) {
    CCVPE_LAUNCH(track_viterbi_back_kernel, dim3(p.B), dim3(256), 0, s, p);
}

}  // namespace ccvpe
