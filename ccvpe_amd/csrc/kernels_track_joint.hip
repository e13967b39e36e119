// Joint position-heading filter (ccvpe_track_joint_predict, ccvpe_track_joint_update_logits): a histogram filter over
// (heading bin k, cell i).  The state is one [512][512] map per heading bin, joint [B][nb][512*512], linear and non-negative.
//
// Predict, per query (w = 360 / nb, th the one-sided heading taps, P(m; d) = track_predict_kernel's c for a map m and a shift d):
//
//     A(k', .)  = P(joint[k']; shift[k'])                                  the motion of every SOURCE bin
//     u0        = -turn_deg / w  (float64),  o = floor(u0),  f = (float)(u0 - o)
//     M[d]      = fmaf(f, th[|d - 1|], (1 - f) * th[|d|])                  d = -rh .. rh + 1   (th = 0 outside 0..rh)
//     C(k, i)   = sum over d, ascending, of fmaf(M[d], A((k + o + d) mod nb, i), C)
//     prior     = C + floor
//
// which is g(k) = (1 - f) A(k + o) + f A(k + o + 1) blurred with th[|j|] on the circle, the linear weights folded into the 2 rh + 2
// merged weights as the xy passes fold the bilinear ones.  f == 0 gives M[d] = th[|d|] exactly.  Two launches:
//   track_joint_xy_kernel   (256 tiles, B * nb)  track_blur.h's staging and passes on slice s = b * nb + k'; c stored to `work`
//   track_joint_mix_kernel  (1024 groups, B)     a group of 256 cells: the nb float4 of every cell quad staged in LDS once (1 KB
//                                                coalesced per slice and wave), then wave v the bins v, v + 4, ..: 2 rh + 2
//                                                ds_read_b128 and 4 (2 rh + 2) fused multiply-adds per float4 of output
// LDS: xy as track_predict_kernel; mix nb KB + the weights (72.3 KB at nb = 72: two workgroups per CU).  `work` is read once and
// `prior` written once.  No input value moves a read outside the tensors: the xy pass clamps and guards as track_predict_kernel, and
// the integer part of the turn is clamped to +-2^30 before it is converted and reduced modulo nb.
//
// Update, per query (e the emission table, m the largest logit by the softmax statistics):
//
//     w_i = __expf(l_i - m),  E(k | i) = valid(c_i, s_i) ? e[(k - bin(c_i, s_i)) mod nb] : e[nb]
//     U(k, i) = (w_i * E(k | i)) * prior(k, i),  Z = float64 sum of U,  J' = U * (float)(1 / Z)
//     (Z not finite, zero, or without a finite float32 reciprocal: no posterior - zeros and the row (-1, NaN, -1, m, Z))
//
// Four launches; the hand-offs are the launch boundaries:
//   softmax_partial_kernel     (64 chunks, B)  the statistics of the logits (kernels_tail.hip)
//   track_joint_sum_kernel     (64 chunks, B)  m; per thread 16 cells' (w, bin) once, then the bins in turn, the next bin's prior
//                                              requested before the work on this one: the chunk's sum of U
//   track_joint_store_kernel   (64 chunks, B)  Z from the 64 chunk sums; U again (the same expression, the same bits), J' stored, the
//                                              marginal in ascending k, the chunk's sum of J' per bin and its (max, first index)
//   track_joint_finish_kernel  (B)             hist from the chunk sums, the marginal's argmax, the best bin there, the row
// The joint moves through HBM three times (the prior read twice, J' written once; once without a prior); storing U in the second
// launch and scaling it in the third would move it four times.  Every sum has one order - a thread's values in (k, float4, x..w)
// order, xor shuffles over the wave, waves 0..3 in turn, the 64 chunks as lanes under the xor shuffles - and nothing is accumulated
// with atomics, so the same inputs give the same bits, alone as in a batch.  joint_out may be prior: every (k, cell) is read by the
// thread that later writes it, and the sum launch writes nothing of it.
#include "tail_shared.h"
#include "track_blur.h"

namespace ccvpe {

static constexpr int JOINT_MIX_QUADS = 64;                                         // float4 of cells per mix workgroup: one per lane
static constexpr int JOINT_MIX_GROUPS = TAIL_HW * TAIL_HW / (4 * JOINT_MIX_QUADS);   // 1024 per query

size_t track_joint_work_bytes(int B, int nb) { return sizeof(float) * (size_t)B * (size_t)nb * TAIL_HW * TAIL_HW; }

__global__ __launch_bounds__(256) void track_joint_xy_kernel(const TrackJointPredictParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char jx_smem[];
    constexpr int HW = TAIL_HW, n = HW * HW;
    const int s = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;    // slice s = b * nb + k'
    const int r = p.radius;
    const int b = s / p.nb;
    const int Y0 = (t / (HW / TRACK_T)) * TRACK_T, X0 = (t % (HW / TRACK_T)) * TRACK_T;
    const TrackTile tile = track_tile(jx_smem, r);
    // slice s is map 0 of the batch of maps at joint + s * n, with its own shift and its query's taps
    track_stage_shifted(tile, p.joint + (size_t)s * n, p.shift + (size_t)s * 2, 1.f, p.taps + (size_t)b * p.taps_stride, 0, 0, r, Y0, X0);
    __syncthreads();
    const float4 c = track_blur_passes<1>(tile.src, tile.S, tile.P, tile.mid, tile.wx, tile.wy, r);
    const int cell = (Y0 + (tid >> 3)) * HW + X0 + (tid & 7) * 4;
    *reinterpret_cast<float4*>(p.work + (size_t)s * n + cell) = c;
}

static size_t joint_mix_lds_bytes(int nb, int rh) { return sizeof(float4) * (size_t)nb * JOINT_MIX_QUADS + sizeof(float) * (2 * rh + 2); }

__global__ __launch_bounds__(256) void track_joint_mix_kernel(const TrackJointPredictParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char jm_smem[];
    constexpr int n4 = TAIL_HW * TAIL_HW / 4;
    const int b = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int nb = min(max(p.nb, JOINT_MIN_BINS), JOINT_MAX_BINS);
    const int rh = min(min(max(p.hradius, 0), TRACK_MAX_R), (nb - 1) / 2);
    float4* A = reinterpret_cast<float4*>(jm_smem);                  // [nb][64] the slices' c at this group's cells
    float* mw = reinterpret_cast<float*>(A + nb * JOINT_MIX_QUADS);  // [2 rh + 2] merged weights, mw[d + rh] = M[d]
    const double u0 = -((double)p.turn_deg[b] / (360.0 / (double)nb));
    const double fl0 = floor(u0);
    const float f = (float)(u0 - fl0);
    // integer part clamped to +-2^30 (fmax returns the clamp for NaN) and reduced modulo nb: no turn moves a read outside the slices
    int o = (int)fmin(fmax(fl0, -1073741824.), 1073741824.) % nb;
    if (o < 0) o += nb;
    if (tid < 2 * rh + 2) {
        const int d = tid - rh;
        const int a = d < 0 ? -d : d, c = d - 1 < 0 ? 1 - d : d - 1;   // |d|, |d - 1|
        const float* th = p.htaps + (size_t)b * p.htaps_stride;
        const float ta = a <= rh ? th[a] : 0.f, tc = c <= rh ? th[c] : 0.f;
        mw[tid] = fmaf(f, tc, (1.f - f) * ta);
    }
    const float4* src = reinterpret_cast<const float4*>(p.work) + (size_t)b * nb * n4 + (size_t)g * JOINT_MIX_QUADS + lane;
    for (int k = wave; k < nb; k += 4) A[k * JOINT_MIX_QUADS + lane] = src[(size_t)k * n4];
    __syncthreads();
    const float fl = p.floor[b];
    float4* dst = reinterpret_cast<float4*>(p.prior) + (size_t)b * nb * n4 + (size_t)g * JOINT_MIX_QUADS + lane;
    for (int k = wave; k < nb; k += 4) {
        int j = k + o - rh;                                          // in (-nb, 2 nb): the first source bin, on the circle
        if (j < 0) j += nb;
        if (j >= nb) j -= nb;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int d = 0; d <= 2 * rh + 1; ++d) {
            const float4 v = A[j * JOINT_MIX_QUADS + lane];
            const float w = mw[d];
            a.x = fmaf(w, v.x, a.x); a.y = fmaf(w, v.y, a.y); a.z = fmaf(w, v.z, a.z); a.w = fmaf(w, v.w, a.w);
            if (++j == nb) j = 0;
        }
        dst[(size_t)k * n4] = make_float4(a.x + fl, a.y + fl, a.z + fl, a.w + fl);
    }
}

void launch_track_joint_predict(const TrackJointPredictParams& p, hipStream_t s) {
    const size_t lds = track_lds_bytes(p.radius), mix_lds = joint_mix_lds_bytes(p.nb, p.hradius);
    static LdsAttr xy_attr, mix_attr;
    ensure_dynamic_lds(xy_attr, reinterpret_cast<const void*>(track_joint_xy_kernel), lds);
    ensure_dynamic_lds(mix_attr, reinterpret_cast<const void*>(track_joint_mix_kernel), mix_lds);
    CCVPE_LAUNCH(track_joint_xy_kernel, dim3(TRACK_TILES, p.B * p.nb), dim3(256), lds, s, p);
    CCVPE_LAUNCH(track_joint_mix_kernel, dim3(JOINT_MIX_GROUPS, p.B), dim3(256), mix_lds, s, p);
}

void launch_track_joint_xy(const TrackJointPredictParams& p, hipStream_t s) {
    const size_t lds = track_lds_bytes(p.radius);
    static LdsAttr xy_attr;
    ensure_dynamic_lds(xy_attr, reinterpret_cast<const void*>(track_joint_xy_kernel), lds);
    CCVPE_LAUNCH(track_joint_xy_kernel, dim3(TRACK_TILES, p.B * p.nb), dim3(256), lds, s, p);
}

void launch_track_joint_mix(const TrackJointPredictParams& p, hipStream_t s) {
    const size_t mix_lds = joint_mix_lds_bytes(p.nb, p.hradius);
    // the kernel's largest size, asked for on every call: launch_track_joint_predict keeps a record of its own for this kernel, so a
    // smaller request from either side after a larger one from the other would leave a record stale
    LdsAttr mix_attr;
    ensure_dynamic_lds(mix_attr, reinterpret_cast<const void*>(track_joint_mix_kernel), joint_mix_lds_bytes(JOINT_MAX_BINS, TRACK_MAX_R));
    CCVPE_LAUNCH(track_joint_mix_kernel, dim3(JOINT_MIX_GROUPS, p.B), dim3(256), mix_lds, s, p);
}

// ---- update ----------------------------------------------------------------------------------------------------------------------

size_t track_joint_scratch_bytes(int B) {
    return (size_t)B * (sizeof(double) * (JOINT_MAX_BINS + 1) * TAIL_CHUNKS + sizeof(float) * 4 * TAIL_CHUNKS);
}
void track_joint_scratch(void* scratch, int cap, TrackJointUpdateParams& p) {
    p.hpart = reinterpret_cast<double*>(scratch);
    p.zpart = p.hpart + (size_t)cap * JOINT_MAX_BINS * TAIL_CHUNKS;
    p.pairs = reinterpret_cast<float*>(p.zpart + (size_t)cap * TAIL_CHUNKS);
    p.partial = p.pairs + (size_t)cap * TAIL_CHUNKS * 2;
}

// A thread's 16 cells of a chunk - four float4, TAIL_CHUNKS' layout - as the sum and the store launch hold them: the weight of the
// logit and the heading bin of the field (nb: the cell has no heading).  One definition, so both launches form the same U.
struct JointCells {
    float w[16];
    int bin[16];
};
__device__ __forceinline__ void joint_cells(const TrackJointUpdateParams& p, int b, int lo, float m, int nb, JointCells& jc) {
    constexpr int n = TAIL_HW * TAIL_HW;
    const float scale = (float)nb / 360.f;
    float4 l[4], fc[4], fs[4];
    load_chunk<false>(p.logits + (size_t)b * n, nullptr, lo, l);
    load_chunk<false>(p.ori + (size_t)b * 2 * n, nullptr, lo, fc);
    load_chunk<false>(p.ori + (size_t)b * 2 * n + n, nullptr, lo, fs);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const float lv[4] = {l[u].x, l[u].y, l[u].z, l[u].w}, cv[4] = {fc[u].x, fc[u].y, fc[u].z, fc[u].w}, sv[4] = {fs[u].x, fs[u].y, fs[u].z, fs[u].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            jc.w[u * 4 + e] = __expf(lv[e] - m);
            jc.bin[u * 4 + e] = heading_valid(cv[e], sv[e]) ? heading_bin(cv[e], sv[e], scale, nb) : nb;
        }
    }
}
// U of bin k at the thread's float4 u: em [nb + 1] the query's emission table in LDS, q the prior there (1 without one)
__device__ __forceinline__ float joint_u(const JointCells& jc, int i, const float* em, int k, int nb, float q) {
    const int bin = jc.bin[i];
    int j = k - bin;
    if (j < 0) j += nb;
    const float e = em[bin == nb ? nb : j];
    return (jc.w[i] * e) * q;
}
// the prior of bin k at the thread's 16 cells (1 without one); the loops ask for bin k + 1 before they work on bin k
template <bool PRIOR>
__device__ __forceinline__ void joint_prior(const TrackJointUpdateParams& p, int b, int k, int nb, int lo, float4 (&q)[4]) {
    constexpr int n = TAIL_HW * TAIL_HW;
    if constexpr (PRIOR) {
        load_chunk<false>(p.prior + ((size_t)b * nb + k) * n, nullptr, lo, q);
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = make_float4(1.f, 1.f, 1.f, 1.f);
    }
}
__device__ __forceinline__ void joint_u_bin(const JointCells& jc, const float* em, int k, int nb, const float4 (&q)[4], float4 (&U)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
        U[u] = make_float4(joint_u(jc, u * 4 + 0, em, k, nb, q[u].x), joint_u(jc, u * 4 + 1, em, k, nb, q[u].y),
                           joint_u(jc, u * 4 + 2, em, k, nb, q[u].z), joint_u(jc, u * 4 + 3, em, k, nb, q[u].w));
}

template <bool PRIOR>
__global__ __launch_bounds__(256) void track_joint_sum_kernel(const TrackJointUpdateParams p) {
    __shared__ float gm, gs;
    __shared__ float em[JOINT_MAX_BINS + 1];
    __shared__ double red[4];
    const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x;
    const int nb = min(max(p.nb, JOINT_MIN_BINS), JOINT_MAX_BINS);
    const int lo = ch * (TAIL_HW * TAIL_HW / TAIL_CHUNKS);
    softmax_stats(p.partial, b, TAIL_CHUNKS, gm, gs);
    if (tid >= 64 && tid < 64 + nb + 1) em[tid - 64] = p.emission[(size_t)b * p.emission_stride + tid - 64];
    __syncthreads();
    JointCells jc;
    joint_cells(p, b, lo, gm, nb, jc);
    double acc[1] = {0.0};
    float4 q[4], qn[4];
    joint_prior<PRIOR>(p, b, 0, nb, lo, q);
    for (int k = 0; k < nb; ++k) {
        float4 U[4];
        joint_prior<PRIOR>(p, b, min(k + 1, nb - 1), nb, lo, qn);
        joint_u_bin(jc, em, k, nb, q, U);
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = qn[u];
#pragma unroll
        for (int u = 0; u < 4; ++u) { acc[0] += (double)U[u].x; acc[0] += (double)U[u].y; acc[0] += (double)U[u].z; acc[0] += (double)U[u].w; }
    }
    summ_wave_to_lds<1>(acc, red);
    __syncthreads();
    if (tid == 0) {
        summ_from_lds<1>(acc, red);
        p.zpart[(size_t)b * TAIL_CHUNKS + ch] = acc[0];
    }
}

// the query's sum from its 64 chunk sums, every lane of the first wave: lane = chunk, then the xor shuffles
__device__ __forceinline__ double joint_sum_chunks(const double* part) {
    double v = part[threadIdx.x & 63];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// A query has a joint posterior when Z is finite and positive and (float)(1 / Z) is finite as well (a positive Z below 2^-128 has no
// float32 reciprocal); the store and the finish launch decide by this one expression
__device__ __forceinline__ bool joint_good(double Z) { return isfinite(Z) && Z > 0.0 && isfinite((float)(1.0 / Z)); }

template <bool PRIOR>
__global__ __launch_bounds__(256) void track_joint_store_kernel(const TrackJointUpdateParams p) {
    __shared__ float gm, gs;
    __shared__ float em[JOINT_MAX_BINS + 1];
    __shared__ double zs;
    __shared__ double hw[JOINT_MAX_BINS][4];
    __shared__ float sv[4];
    __shared__ int si[4];
    constexpr int n = TAIL_HW * TAIL_HW;
    const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x;
    const int nb = min(max(p.nb, JOINT_MIN_BINS), JOINT_MAX_BINS);
    const int lo = ch * (n / TAIL_CHUNKS);
    softmax_stats(p.partial, b, TAIL_CHUNKS, gm, gs);
    if (tid < 64) {
        const double Z = joint_sum_chunks(p.zpart + (size_t)b * TAIL_CHUNKS);
        if (tid == 0) zs = Z;
    }
    if (tid >= 64 && tid < 64 + nb + 1) em[tid - 64] = p.emission[(size_t)b * p.emission_stride + tid - 64];
    __syncthreads();
    const double Z = zs;
    const float inv = (float)(1.0 / Z);
    const bool good = joint_good(Z);                   // else: a query without a finite joint posterior, all zero
    JointCells jc;
    joint_cells(p, b, lo, gm, nb, jc);
    float4 mg[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) mg[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 q[4], qn[4];
    joint_prior<PRIOR>(p, b, 0, nb, lo, q);
    for (int k = 0; k < nb; ++k) {
        float4 U[4];
        joint_prior<PRIOR>(p, b, min(k + 1, nb - 1), nb, lo, qn);
        joint_u_bin(jc, em, k, nb, q, U);
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = qn[u];
        float4* dst = reinterpret_cast<float4*>(p.joint_out + ((size_t)b * nb + k) * n + lo);
        double h[1] = {0.0};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float4 J = good ? make_float4(U[u].x * inv, U[u].y * inv, U[u].z * inv, U[u].w * inv) : make_float4(0.f, 0.f, 0.f, 0.f);
            dst[tid + u * 256] = J;
            mg[u].x += J.x; mg[u].y += J.y; mg[u].z += J.z; mg[u].w += J.w;
            h[0] += (double)J.x; h[0] += (double)J.y; h[0] += (double)J.z; h[0] += (double)J.w;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) h[0] += __shfl_xor(h[0], off);
        if ((tid & 63) == 0) hw[k][tid >> 6] = h[0];
    }
    float4* md = reinterpret_cast<float4*>(p.marginal + (size_t)b * n + lo);
    float best = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        md[tid + u * 256] = mg[u];
        // the next address reuses this store's registers at once: two wait states behind the 16-byte store, as in kernels_level6.hip
        // (tests/test_isa_hazard.py checks the generated code)
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 1");
        __builtin_amdgcn_sched_barrier(0);
        const int cell = lo + (tid + u * 256) * 4;
        argmax_merge(best, bi, mg[u].x, cell);
        argmax_merge(best, bi, mg[u].y, cell + 1);
        argmax_merge(best, bi, mg[u].z, cell + 2);
        argmax_merge(best, bi, mg[u].w, cell + 3);
    }
    argmax_wave(best, bi);
    if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < 4; ++v) argmax_merge(best, bi, sv[v], si[v]);
        float* pair = p.pairs + ((size_t)b * TAIL_CHUNKS + ch) * 2;
        pair[0] = best;
        pair[1] = __int_as_float(bi);
    }
    if (tid < nb) p.hpart[((size_t)b * JOINT_MAX_BINS + tid) * TAIL_CHUNKS + ch] = ((hw[tid][0] + hw[tid][1]) + hw[tid][2]) + hw[tid][3];
}

// Grid (B), 256 threads: wave v totals the bins v, v + 4, ..; the first wave the marginal's argmax and, with it, the row
__global__ __launch_bounds__(256) void track_joint_finish_kernel(const TrackJointUpdateParams p) {
    __shared__ float gm, gs;
    constexpr int n = TAIL_HW * TAIL_HW;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int nb = min(max(p.nb, JOINT_MIN_BINS), JOINT_MAX_BINS);
    softmax_stats(p.partial, b, TAIL_CHUNKS, gm, gs);
    for (int k = wave; k < nb; k += 4) {
        const double v = joint_sum_chunks(p.hpart + ((size_t)b * JOINT_MAX_BINS + k) * TAIL_CHUNKS);
        if (lane == 0) p.hist[(size_t)b * nb + k] = (float)v;
    }
    __syncthreads();
    if (tid < 64) {
        const double Z = joint_sum_chunks(p.zpart + (size_t)b * TAIL_CHUNKS);
        const float* pr = p.pairs + ((size_t)b * TAIL_CHUNKS + lane) * 2;
        float best = pr[0];
        int bi = __float_as_int(pr[1]);
        argmax_wave(best, bi);
        if (tid == 0) {
            const bool good = joint_good(Z) && best > -INFINITY && (unsigned)bi < (unsigned)n;
            float* row = p.rows + (size_t)b * JOINT_COLS;
            int bk = -1;
            if (good) {
                float bv = -INFINITY;
                for (int k = 0; k < nb; ++k) {
                    const float v = p.joint_out[((size_t)b * nb + k) * n + bi];
                    if (v > bv) { bv = v; bk = k; }          // (the first of equal values)
                }
            }
            row[0] = good ? (float)bi : -1.f;
            row[1] = good ? best : NAN;
            row[2] = (float)bk;
            row[3] = gm;
            row[4] = (float)Z;
        }
    }
}

void launch_track_joint_update(const TrackJointUpdateParams& p, hipStream_t s) {
    SoftmaxParams sp{};
    sp.logits = p.logits; sp.B = p.B; sp.n = TAIL_HW * TAIL_HW; sp.partial = p.partial; sp.chunks = TAIL_CHUNKS;
    launch_softmax_partial(sp, s);
    if (p.prior) {
        CCVPE_LAUNCH(track_joint_sum_kernel<true>, dim3(TAIL_CHUNKS, p.B), dim3(256), 0, s, p);
        CCVPE_LAUNCH(track_joint_store_kernel<true>, dim3(TAIL_CHUNKS, p.B), dim3(256), 0, s, p);
    } else {
        CCVPE_LAUNCH(track_joint_sum_kernel<false>, dim3(TAIL_CHUNKS, p.B), dim3(256), 0, s, p);
        CCVPE_LAUNCH(track_joint_store_kernel<false>, dim3(TAIL_CHUNKS, p.B), dim3(256), 0, s, p);
    }
    CCVPE_LAUNCH(track_joint_finish_kernel, dim3(p.B), dim3(256), 0, s, p);
}

}  // namespace ccvpe
