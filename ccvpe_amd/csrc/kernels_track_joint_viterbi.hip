// MAP trajectory of a joint position-heading stream (ccvpe_track_joint_viterbi, ccvpe_track_joint_viterbi_back): the
// max-product sweep over the stored joints of the histogram filter over (heading bin k, cell i), with the filter's own transition read
// as a latent choice per link - the source bin offset d (which of the 2 rh + 2 merged circle weights carried the mass), the window
// position (as in kernels_track_viterbi.hip), or a jump through the relocalisation floor to any state.  Per query, with J the filter
// joint of frame t, J- that of frame t - 1, v- the score joint of frame t - 1 and shift, taps, turn_deg, htaps, floor the arguments of
// the ccvpe_track_joint_predict call between the two (P(m; d), o, f and M[d] as in kernels_track_joint.hip; ux, uy the merged weights
// of track_stage_shifted under shift[k']):
//
//     A(k')      = P(J-[k']; shift[k'])                                      the predict's first launch, unedited
//     prior(k,i) = (fmaf chain of M[d] A((k + o + d) mod nb, i), ascending d) + floor       the bits the predict stores
//     lik(k,i)   = J(k,i) > 0 ? J(k,i) / prior(k,i) : 0
//     win(k',i)  = max_ky fl(uy[ky] * max_kx fl(ux[kx] * v-(k', source cell)))              per SOURCE bin, under shift[k']
//     mix(k,i)   = max over d = -rh..rh+1 of fl(M[d] * win((k + o + d) mod nb, i))
//     m(k,i)     = max(mix(k,i), fl(floor * v-(jk, j)))                      (jk, j): the first index of the largest v- (prev_stats)
//     w          = fl(lik * m), a w that is not > 0 stored as 0
//     v          = ldexpf(w, -e),  W = max over (k, i) of w at its first flat index k n + i,  W * 2^-e in [1, 2)      one e per query
//
// Every maximum takes its candidates as `c > acc ? c : acc` from 0 (maxmul_take): NaN and negative products never enter.  Four launches
// per step and one per backtracked link; the hand-offs are the launch boundaries, no atomics, no counters, no scratch:
//   track_joint_xy_kernel            (256 tiles, B nb)  kernels_track_joint.hip's, on J- into `work`: A
//   track_joint_viterbi_win_kernel   (256 tiles, B nb)  track_stage_shifted of v-[k'] under shift[k'] and the two max passes of
//                                                       track_maxmul.h; win to the second joint of `work`.  A restarted query's
//                                                       workgroups return at once.
//   track_joint_viterbi_mix_kernel   (1024 groups, B)   the mix and ratio kernels' grid and staging: A's nb float4 per cell quad in LDS,
//                                                       the prior with the mix kernel's statements, lik of a wave's <= 18 bins held in
//                                                       registers, a barrier, the same LDS restaged with win, the circle max over d, the
//                                                       jump, the product and the clean; w to `score`, the group's (max, first flat
//                                                       index) to `work`
//   track_joint_viterbi_scale_kernel (16 parts, B nb)   W and its first index from the 1024 group pairs; the slice scaled in place by
//                                                       2^-e, or zeroed; the stats row
//   track_joint_viterbi_back_kernel  (B)                the (2 rh + 2)(2 r + 2)^2 candidates of one (cell, bin) straight from global
//                                                       memory, every read guarded
// The first frame (no J-) is the mix and the scale launch alone, w = J cleaned; a restart (no valid (cell, bin) in prev_stats, or v-
// there not > 0) stores lik and skips the second staging.  The joint moves through HBM ten times: 2 (xy) + 2 (win) + 4 (mix: A, win, J
// read, w written) + 2 (scale).  LDS of the mix launch: nb KB + the weights, 72.3 KB at nb = 72, two workgroups per CU as the mix
// kernel; 160 VGPRs, of which 72 hold lik (the ratio kernel's layout: a second LDS buffer instead was 1.76 times slower there), 66
// SGPRs, no scratch: three waves per SIMD by registers, so three workgroups per CU up to nb 53 and two by LDS (160 KB per CU) beyond.
// The recursion has no sum of its own beyond the prior's and the scaling is by a power of two, so the same inputs give the same bits,
// alone as in a batch.  No input value moves a read outside a tensor: the xy and win launches clamp and guard as track_predict_kernel,
// the mix launch clamps the integer part of the turn as the mix kernel does, and prev_stats is guarded for cell < n and bin < nb.
#include "tail_shared.h"
#include "track_maxmul.h"

namespace ccvpe {

static constexpr int JV_QUADS = 64;                                        // float4 of cells per mix workgroup: one per lane
static constexpr int JV_GROUPS = TAIL_HW * TAIL_HW / (4 * JV_QUADS);       // 1024 per query
static constexpr int JV_BINS_PER_WAVE = (JOINT_MAX_BINS + 3) / 4;          // 18: the bins wave, wave + 4, .. of a mix workgroup
static constexpr int JV_PARTS = 16;                                        // scale workgroups per slice: 16384 cells each

// `work`: A [B][nb][n], win [B][nb][n], then the groups' pairs [B][1024][2] (max, first flat index as int bits)
size_t track_joint_viterbi_work_bytes(int B, int nb) {
    return sizeof(float) * (2 * (size_t)B * (size_t)nb * TAIL_HW * TAIL_HW + (size_t)B * JV_GROUPS * 2);
}
__device__ __forceinline__ float* joint_viterbi_win(float* work, int B, int nb) { return work + (size_t)B * nb * TAIL_HW * TAIL_HW; }
__device__ __forceinline__ float* joint_viterbi_pairs(float* work, int B, int nb) { return work + 2 * (size_t)B * nb * TAIL_HW * TAIL_HW; }

// The flat index jk n + j of prev_stats' (cell, bin) when both are inside the grid, else -1 (NaN fails every comparison)
__device__ __forceinline__ int joint_viterbi_prev_index(const float* prev_stats, int b, int nb) {
    constexpr int n = TAIL_HW * TAIL_HW;
    const float c = prev_stats[(size_t)b * JOINT_VITERBI_COLS], k = prev_stats[(size_t)b * JOINT_VITERBI_COLS + 1];
    return c >= 0.f && c < (float)n && k >= 0.f && k < (float)nb ? (int)k * n + (int)c : -1;
}
// v- at prev_stats' pair, 0 without one: a query restarts when this is not > 0.  One expression for the win, mix and scale launches.
__device__ __forceinline__ float joint_viterbi_peak(const float* score_prev, const float* prev_stats, int b, int nb) {
    const int j = joint_viterbi_prev_index(prev_stats, b, nb);
    return j >= 0 ? score_prev[(size_t)b * nb * (TAIL_HW * TAIL_HW) + j] : 0.f;
}

// o and f of a turn: track_joint_mix_kernel's statements
struct JointTurn { int o; float f; };
__device__ __forceinline__ JointTurn joint_viterbi_turn(float turn_deg, int nb) {
    const double u0 = -((double)turn_deg / (360.0 / (double)nb));
    const double fl0 = floor(u0);
    JointTurn t;
    t.f = (float)(u0 - fl0);
    // integer part clamped to +-2^30 (fmax returns the clamp for NaN) and reduced modulo nb: no turn moves a read outside the slices
    t.o = (int)fmin(fmax(fl0, -1073741824.), 1073741824.) % nb;
    if (t.o < 0) t.o += nb;
    return t;
}
// M[d], d = i - rh, i = 0 .. 2 rh + 1: track_joint_mix_kernel's statements
__device__ __forceinline__ float joint_viterbi_circle_weight(const float* th, int rh, float f, int i) {
    const int d = i - rh;
    const int a = d < 0 ? -d : d, c = d - 1 < 0 ? 1 - d : d - 1;   // |d|, |d - 1|
    const float ta = a <= rh ? th[a] : 0.f, tc = c <= rh ? th[c] : 0.f;
    return fmaf(f, tc, (1.f - f) * ta);
}

__global__ __launch_bounds__(256) void track_joint_viterbi_win_kernel(const TrackJointViterbiParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char jvw_smem[];
    constexpr int HW = TAIL_HW, n = HW * HW;
    const int s = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;    // slice s = b * nb + k'
    const int r = p.radius;
    const int nb = min(max(p.nb, JOINT_MIN_BINS), JOINT_MAX_BINS);
    const int b = s / nb;
    if (!(joint_viterbi_peak(p.score_prev, p.prev_stats, b, nb) > 0.f)) return;   // a restart: the same for every thread of the query
    const int Y0 = (t / (HW / TRACK_T)) * TRACK_T, X0 = (t % (HW / TRACK_T)) * TRACK_T;
    const TrackTile tile = track_tile(jvw_smem, r);
    // slice s is map 0 of the batch of maps at score_prev + s * n, with its own shift and its query's taps
    track_stage_shifted(tile, p.score_prev + (size_t)s * n, p.shift + (size_t)s * 2, 1.f, p.taps + (size_t)b * p.taps_stride, 0, 0, r, Y0, X0);
    __syncthreads();
    const float4 win = track_maxmul_passes<1>(tile.src, tile.S, tile.P, tile.mid, tile.wx, tile.wy, r);
    const int cell = (Y0 + (tid >> 3)) * HW + X0 + (tid & 7) * 4;
    *reinterpret_cast<float4*>(joint_viterbi_win(p.work, p.B, nb) + (size_t)s * n + cell) = win;
}

__global__ __launch_bounds__(256) void track_joint_viterbi_mix_kernel(const TrackJointViterbiParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char jvm_smem[];
    __shared__ float redv[4];
    __shared__ int redi[4];
    constexpr int n = TAIL_HW * TAIL_HW, n4 = n / 4;
    const int b = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int nb = min(max(p.nb, JOINT_MIN_BINS), JOINT_MAX_BINS);
    const int rh = min(min(max(p.hradius, 0), TRACK_MAX_R), (nb - 1) / 2);
    const bool first = p.joint_prev == nullptr;
    float4* A = reinterpret_cast<float4*>(jvm_smem);                   // [nb][64] the slices' c at this group's cells, then win there
    float* mw = reinterpret_cast<float*>(A + nb * JV_QUADS);           // [2 rh + 2] merged weights, mw[d + rh] = M[d]
    const size_t base = (size_t)b * nb * n4 + (size_t)g * JV_QUADS + lane;
    int o = 0;
    float fl = 0.f, peak = 0.f;
    if (!first) {
        const JointTurn turn = joint_viterbi_turn(p.turn_deg[b], nb);
        o = turn.o;
        if (tid < 2 * rh + 2) mw[tid] = joint_viterbi_circle_weight(p.htaps + (size_t)b * p.htaps_stride, rh, turn.f, tid);
        const float4* src = reinterpret_cast<const float4*>(p.work) + base;
        for (int k = wave; k < nb; k += 4) A[k * JV_QUADS + lane] = src[(size_t)k * n4];
        fl = p.floor[b];
        peak = joint_viterbi_peak(p.score_prev, p.prev_stats, b, nb);
        __syncthreads();
    }
    const float4* cur = reinterpret_cast<const float4*>(p.joint) + base;
    // a thread's bins wave, wave + 4, ..: lik stays in registers (every index a constant of the unrolled loop) until the whole workgroup
    // has formed its priors, then LDS is restaged with win
    float4 q[JV_BINS_PER_WAVE];
#pragma unroll
    for (int i = 0; i < JV_BINS_PER_WAVE; ++i) {
        const int k = wave + 4 * i;
        q[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < nb) {
            const float4 J = cur[(size_t)k * n4];
            if (first) {
                q[i] = J;
            } else {
                int j = k + o - rh;                                    // in (-nb, 2 nb): the first source bin, on the circle
                if (j < 0) j += nb;
                if (j >= nb) j -= nb;
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
                for (int d = 0; d <= 2 * rh + 1; ++d) {
                    const float4 v = A[j * JV_QUADS + lane];
                    const float w = mw[d];
                    a.x = fmaf(w, v.x, a.x); a.y = fmaf(w, v.y, a.y); a.z = fmaf(w, v.z, a.z); a.w = fmaf(w, v.w, a.w);
                    if (++j == nb) j = 0;
                }
                q[i].x = J.x > 0.f ? J.x / (a.x + fl) : 0.f;
                q[i].y = J.y > 0.f ? J.y / (a.y + fl) : 0.f;
                q[i].z = J.z > 0.f ? J.z / (a.z + fl) : 0.f;
                q[i].w = J.w > 0.f ? J.w / (a.w + fl) : 0.f;
            }
        }
    }
    if (!first && peak > 0.f) {                 // the same for every thread of the query; else a restart: m = 1
        __syncthreads();                        // every prior is formed: A has been read
        const float4* src = reinterpret_cast<const float4*>(joint_viterbi_win(p.work, p.B, nb)) + base;
        for (int k = wave; k < nb; k += 4) A[k * JV_QUADS + lane] = src[(size_t)k * n4];
        __syncthreads();
        const float jump = fl * peak;
#pragma unroll
        for (int i = 0; i < JV_BINS_PER_WAVE; ++i) {
            const int k = wave + 4 * i;
            if (k < nb) {
                int j = k + o - rh;
                if (j < 0) j += nb;
                if (j >= nb) j -= nb;
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
                for (int d = 0; d <= 2 * rh + 1; ++d) {
                    const float4 v = A[j * JV_QUADS + lane];
                    const float w = mw[d];
                    a.x = maxmul_take(a.x, w * v.x); a.y = maxmul_take(a.y, w * v.y); a.z = maxmul_take(a.z, w * v.z); a.w = maxmul_take(a.w, w * v.w);
                    if (++j == nb) j = 0;
                }
                q[i].x = q[i].x * (jump > a.x ? jump : a.x);
                q[i].y = q[i].y * (jump > a.y ? jump : a.y);
                q[i].z = q[i].z * (jump > a.z ? jump : a.z);
                q[i].w = q[i].w * (jump > a.w ? jump : a.w);
            }
        }
    }
    float4* dst = reinterpret_cast<float4*>(p.score) + base;
    float best = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < JV_BINS_PER_WAVE; ++i) {
        const int k = wave + 4 * i;
        if (k < nb) {
            const float4 w = make_float4(viterbi_clean(q[i].x), viterbi_clean(q[i].y), viterbi_clean(q[i].z), viterbi_clean(q[i].w));
            dst[(size_t)k * n4] = w;
            // the flat index reuses this store's address registers at once: two wait states behind the 16-byte store, as in
            // kernels_track_joint.hip (tests/test_isa_hazard.py checks the generated code)
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_nop 1");
            __builtin_amdgcn_sched_barrier(0);
            const int flat = k * n + (g * JV_QUADS + lane) * 4;
            argmax_merge(best, bi, w.x, flat);
            argmax_merge(best, bi, w.y, flat + 1);
            argmax_merge(best, bi, w.z, flat + 2);
            argmax_merge(best, bi, w.w, flat + 3);
        }
    }
    argmax_wave(best, bi);
    if (lane == 0) { redv[wave] = best; redi[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < 4; ++v) argmax_merge(best, bi, redv[v], redi[v]);
        float* pair = joint_viterbi_pairs(p.work, p.B, nb) + ((size_t)b * JV_GROUPS + g) * 2;
        pair[0] = best;
        pair[1] = __int_as_float(bi);
    }
}

__global__ __launch_bounds__(256) void track_joint_viterbi_scale_kernel(const TrackJointViterbiParams p) {
    __shared__ float sv[4];
    __shared__ int si[4];
    constexpr int n = TAIL_HW * TAIL_HW;
    const int s = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;    // slice s = b * nb + k
    const int nb = min(max(p.nb, JOINT_MIN_BINS), JOINT_MAX_BINS);
    const int b = s / nb;
    // W and its first flat index from the query's 1024 group pairs: four per thread, the wave, the four waves
    const float* pairs = joint_viterbi_pairs(p.work, p.B, nb) + (size_t)b * JV_GROUPS * 2;
    float W = -INFINITY;
    int bi = 0x7fffffff;
    for (int v = 0; v < JV_GROUPS / 256; ++v) argmax_merge(W, bi, pairs[(tid + v * 256) * 2], __float_as_int(pairs[(tid + v * 256) * 2 + 1]));
    argmax_wave(W, bi);
    if ((tid & 63) == 0) { sv[tid >> 6] = W; si[tid >> 6] = bi; }
    __syncthreads();
    W = sv[0]; bi = si[0];
    for (int v = 1; v < 4; ++v) argmax_merge(W, bi, sv[v], si[v]);
    const bool good = W > 0.f && isfinite(W) && (unsigned)bi < (unsigned)(nb * n);
    // e with W * 2^-e in [1, 2), from the bits: a subnormal W has its leading bit at 31 - clz
    const unsigned bits = __float_as_uint(W);
    const int ex = (int)((bits >> 23) & 0xff);
    const int e = ex ? ex - 127 : (31 - __clz((int)(bits & 0x7fffff))) - 149;
    float4* m = reinterpret_cast<float4*>(p.score + (size_t)s * n + (size_t)part * (n / JV_PARTS));
    for (int c = 0; c < n / JV_PARTS / 4096; ++c) {
        float4* mc = m + c * 1024;
        if (good) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = mc[tid + u * 256];
#pragma unroll
            for (int u = 0; u < 4; ++u) mc[tid + u * 256] = make_float4(ldexpf(v[u].x, -e), ldexpf(v[u].y, -e), ldexpf(v[u].z, -e), ldexpf(v[u].w, -e));
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) mc[tid + u * 256] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    if (part == 0 && s == b * nb && tid == 0) {
        const bool restarted = p.joint_prev == nullptr || !(joint_viterbi_peak(p.score_prev, p.prev_stats, b, nb) > 0.f);
        float* st = p.stats + (size_t)b * JOINT_VITERBI_COLS;
        st[0] = good ? (float)(bi % n) : -1.f;
        st[1] = good ? (float)(bi / n) : -1.f;
        st[2] = good ? ldexpf(W, -e) : NAN;
        st[3] = good ? (float)e : NAN;
        st[4] = restarted ? 1.f : 0.f;
    }
}

static size_t joint_viterbi_mix_lds_bytes(int nb, int rh) { return sizeof(float4) * (size_t)nb * JV_QUADS + sizeof(float) * (2 * rh + 2); }

void launch_track_joint_viterbi(const TrackJointViterbiParams& p, hipStream_t s) {
    static LdsAttr win_attr, mix_attr;
    if (p.joint_prev) {
        TrackJointPredictParams xy{};
        xy.joint = p.joint_prev; xy.shift = p.shift; xy.taps = p.taps; xy.taps_stride = p.taps_stride; xy.radius = p.radius; xy.work = p.work;
        xy.B = p.B; xy.nb = p.nb;
        launch_track_joint_xy(xy, s);
        const size_t lds = track_lds_bytes(p.radius);
        ensure_dynamic_lds(win_attr, reinterpret_cast<const void*>(track_joint_viterbi_win_kernel), lds);
        CCVPE_LAUNCH(track_joint_viterbi_win_kernel, dim3(TRACK_TILES, p.B * p.nb), dim3(256), lds, s, p);
    }
    const size_t mix_lds = joint_viterbi_mix_lds_bytes(p.nb, p.joint_prev ? p.hradius : 0);
    ensure_dynamic_lds(mix_attr, reinterpret_cast<const void*>(track_joint_viterbi_mix_kernel), mix_lds);
    CCVPE_LAUNCH(track_joint_viterbi_mix_kernel, dim3(JV_GROUPS, p.B), dim3(256), mix_lds, s, p);
    CCVPE_LAUNCH(track_joint_viterbi_scale_kernel, dim3(JV_PARTS, p.B * p.nb), dim3(256), 0, s, p);
}

// One link of the backtrack: the source (cell, bin) the path's (cell, bin) of frame t came from, and the link's kind.  One workgroup
// per query; the source bins k' = (bin + o + d) mod nb in turn, thread tid the candidates tid, tid + 256, .. of the (2r + 2)^2 window
// of k' under shift[k'] in raster order.  Every read is guarded: the previous pair by joint_viterbi_prev_index, cell and bin against
// the grid, a candidate's source against the grid; the turn and the shifts clamp as in the step.
__global__ __launch_bounds__(256) void track_joint_viterbi_back_kernel(const TrackJointViterbiBackParams p) {
    __shared__ float redv[4];
    __shared__ int redi[4];
    __shared__ float mw[2 * TRACK_MAX_R + 2];
    constexpr int HW = TAIL_HW, n = HW * HW;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nb = min(max(p.nb, JOINT_MIN_BINS), JOINT_MAX_BINS);
    const int rh = min(min(max(p.hradius, 0), TRACK_MAX_R), (nb - 1) / 2);
    const int cell = p.cell[b], bin = p.bin[b];
    const int j = joint_viterbi_prev_index(p.prev_stats, b, nb);
    int* out = p.back + (size_t)b * 3;
    const bool outside = (unsigned)cell >= (unsigned)n || (unsigned)bin >= (unsigned)nb;
    if (outside || j < 0) {       // the end of a backtrack or the frame behind a broken one; no j: nothing to point at
        if (tid == 0) {
            const bool to_prev = outside && j >= 0;
            out[0] = to_prev ? j % n : -1;
            out[1] = to_prev ? j / n : -1;
            out[2] = VITERBI_LINK_START;
        }
        return;
    }
    const int r = min(max(p.radius, 0), TRACK_MAX_R), K = 2 * r + 2;
    const float* prev = p.score_prev + (size_t)b * nb * n;
    const float* taps = p.taps + (size_t)b * p.taps_stride;
    const JointTurn turn = joint_viterbi_turn(p.turn_deg[b], nb);
    if (tid < 2 * rh + 2) mw[tid] = joint_viterbi_circle_weight(p.htaps + (size_t)b * p.htaps_stride, rh, turn.f, tid);
    __syncthreads();
    int ks = bin + turn.o - rh;                                        // in (-nb, 2 nb): the first source bin, on the circle
    if (ks < 0) ks += nb;
    if (ks >= nb) ks -= nb;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int d = 0; d <= 2 * rh + 1; ++d) {
        const float M = mw[d];
        const float* sh = p.shift + ((size_t)b * nb + ks) * 2;
        const ShiftAxis ax = track_shift_axis(sh[0]), ay = track_shift_axis(sh[1]);
        const int gx0 = cell % HW - ax.i - r - 1, gy0 = cell / HW - ay.i - r - 1;
        const float* slice = prev + (size_t)ks * n;
        for (int i = tid; i < K * K; i += 256) {
            const int ky = i / K, kx = i - ky * K;
            const int gy = gy0 + ky, gx = gx0 + kx;
            if ((unsigned)gy < (unsigned)HW && (unsigned)gx < (unsigned)HW) {
                const float ux = track_merged_weight(taps, r, ax.f, kx), uy = track_merged_weight(taps, r, ay.f, ky);
                const float inner = ux * slice[gy * HW + gx];
                const float moved = uy * inner;
                argmax_merge(best, bi, M * moved, ks * n + gy * HW + gx);
            }
        }
        if (++ks == nb) ks = 0;
    }
    argmax_wave(best, bi);
    if ((tid & 63) == 0) { redv[tid >> 6] = best; redi[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < 4; ++v) argmax_merge(best, bi, redv[v], redi[v]);
        const float jump = p.floor[b] * prev[j];
        int src = j, kind = VITERBI_LINK_START;
        if (!(best > 0.f) && !(jump > 0.f)) kind = VITERBI_LINK_START;
        else if (jump > best) kind = VITERBI_LINK_JUMP;
        else { src = bi; kind = VITERBI_LINK_MOVE; }
        out[0] = src % n;
        out[1] = src / n;
        out[2] = kind;
    }
}

void launch_track_joint_viterbi_back(const TrackJointViterbiBackParams& p, hipStream_t s) {
    CCVPE_LAUNCH(track_joint_viterbi_back_kernel, dim3(p.B), dim3(256), 0, s, p);
}

}  // namespace ccvpe
