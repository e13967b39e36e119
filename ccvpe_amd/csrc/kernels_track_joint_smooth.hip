// Backward step of the joint position-heading filter (ccvpe_track_joint_smooth): the smoothing half of the histogram
// filter over (heading bin k, cell i).  Per query, with J the filter joint of frame t, s' the smoothed joint of frame t + 1 and shift,
// taps, turn_deg, htaps, floor the arguments of the ccvpe_track_joint_predict call that carried J into frame t + 1 (P(m; d), o, f and
// M[d] as in kernels_track_joint.hip):
//
//     A(k')      = P(J[k']; shift[k'])                                       the predict's first launch, unedited
//     prior(k,i) = (fmaf chain of M[d] A((k + o + d) mod nb, i), ascending d) + floor       the bits the predict stores
//     g(k,i)     = s'(k,i) > 0 ? s'(k,i) / prior(k,i) : 0                    NaN and negative s' are not taken
//     G          = sum over k, i of g                                        float64
//     h(k',i)    = sum over d = -rh..rh+1, ascending, of fmaf(M[d], g((k' - o - d) mod nb, i), h)       the adjoint of the circle mix
//     a(k',i)    = fmaf(floor, (float)G, P(h[k']; -shift[k'])_i)             P with the negated shift is the adjoint of P
//     w          = J * a,  Z = float64 sum of w,  s = w * (float)(1 / Z)
//
// Five launches; the hand-offs are the launch boundaries, nothing is accumulated with atomics:
//   track_joint_xy_kernel             (256 tiles, B nb)  kernels_track_joint.hip's, on J into `work`
//   track_joint_smooth_ratio_kernel   (1024 groups, B)   the mix kernel's grid and staging: A's nb float4 per cell quad in LDS, the
//                                                        prior with the mix kernel's statements, g held in registers until every
//                                                        prior is formed and then put in A's place, h stored over A in `work` (a
//                                                        workgroup reads and writes only its own cells of every bin), the group's
//                                                        sum of g
//   track_joint_smooth_weight_kernel  (256 tiles, B nb)  G from the 1024 group sums; track_blur.h's staging of h[k'] under the negated
//                                                        shift and its passes; w to `smoothed` (G == 0: J itself); the tile's sum of w
//   track_joint_smooth_scale_kernel   (64 chunks, B)     Z from the tile sums; w scaled in place (or zeroed, or J left); the marginal in
//                                                        ascending k, the chunk's sum of s per bin and its (max, first index)
//   track_joint_smooth_finish_kernel  (B)                hist, the marginal's argmax, the best bin there, the stats row
// LDS: ratio nb KB + the weights (72.3 KB at nb = 72: two workgroups per CU, as the mix kernel; 126 VGPRs, of which 72 hold g - a
// second LDS buffer instead, 144.3 KB and one workgroup per CU, took 1004 us against 571 at nb 72, batch 8); weight as
// track_predict_kernel.  The joint moves through HBM ten times: 2 (xy) + 3 (ratio: A, s' read, h written) + 3 (weight: h, J read, w written) + 2 (scale).
// Every sum has one order.  A thread's values in (k, float4, x..w) order, xor shuffles over the wave, waves 0..3 in turn; then
//   G: the 1024 group sums as lane l: p[l] + p[l + 64] + .. + p[l + 960] in ascending index, then the xor shuffles;
//   Z: the nb x 256 tile sums as thread t: p[0][t] + p[1][t] + .. in ascending k, xor shuffles, waves 0..3 in turn;
//   hist: the 64 chunk sums of a bin as lanes under the xor shuffles.
// So the same inputs give the same bits, alone as in a batch.  `smoothed` may be `next`: s' is read by the ratio launch only and
// `smoothed` first written by the weight launch; from there every (k, cell) is read by the thread that later writes it.
// No input value moves a read outside a tensor: the xy and weight launches clamp and guard as track_predict_kernel, the ratio launch
// clamps the integer part of the turn as the mix kernel does.
#include "tail_shared.h"
#include "track_blur.h"

namespace ccvpe {

static constexpr int JS_QUADS = 64;                                        // float4 of cells per ratio workgroup: one per lane
static constexpr int JS_GROUPS = TAIL_HW * TAIL_HW / (4 * JS_QUADS);       // 1024 per query
static constexpr int JS_BINS_PER_WAVE = (JOINT_MAX_BINS + 3) / 4;          // 18: the bins wave, wave + 4, .. of a ratio workgroup

// `work` behind the joint-sized buffer: per-query partial sums, the bins at JOINT_MAX_BINS apart whatever nb is
struct JointSmoothWork {
    double* gpart;   // [B][1024]       the ratio groups' sums of g
    double* wpart;   // [B][72][256]    the weight tiles' sums of w
    double* hpart;   // [B][72][64]     the scale chunks' sums of s per bin
    double* zg;      // [B][2]          (Z, G) as the scale launch formed them
    float* pairs;    // [B][64][2]      (max, first index) of the marginal per chunk
};
static constexpr size_t JS_DOUBLES = JS_GROUPS + (size_t)JOINT_MAX_BINS * TRACK_TILES + (size_t)JOINT_MAX_BINS * TAIL_CHUNKS + 2;
size_t track_joint_smooth_work_bytes(int B, int nb) {
    return sizeof(float) * (size_t)B * (size_t)nb * TAIL_HW * TAIL_HW + (size_t)B * (sizeof(double) * JS_DOUBLES + sizeof(float) * 2 * TAIL_CHUNKS);
}
__host__ __device__ __forceinline__ JointSmoothWork joint_smooth_work(float* work, int B, int nb) {
    JointSmoothWork w;
    w.gpart = reinterpret_cast<double*>(work + (size_t)B * nb * TAIL_HW * TAIL_HW);
    w.wpart = w.gpart + (size_t)B * JS_GROUPS;
    w.hpart = w.wpart + (size_t)B * JOINT_MAX_BINS * TRACK_TILES;
    w.zg = w.hpart + (size_t)B * JOINT_MAX_BINS * TAIL_CHUNKS;
    w.pairs = reinterpret_cast<float*>(w.zg + (size_t)B * 2);
    return w;
}

// G of a query from its 1024 group sums, every lane of the first wave
__device__ __forceinline__ double joint_smooth_sum_groups(const double* part) {
    const int lane = threadIdx.x & 63;
    double v = 0.0;
    for (int i = 0; i < JS_GROUPS / 64; ++i) v += part[lane + i * 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
// 64 partial sums as lanes, every lane of a wave
__device__ __forceinline__ double joint_smooth_sum_chunks(const double* part) {
    double v = part[threadIdx.x & 63];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
// The smoothed joint exists when Z is finite and positive and (float)(1 / Z) is finite as well; the scale and the finish launch decide
// by this one expression (the joint filter's rule, kernels_track_joint.hip)
__device__ __forceinline__ bool joint_smooth_good(double Z) { return isfinite(Z) && Z > 0.0 && isfinite((float)(1.0 / Z)); }

__global__ __launch_bounds__(256) void track_joint_smooth_ratio_kernel(const TrackJointSmoothParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char jr_smem[];
    __shared__ double red[4];
    constexpr int n4 = TAIL_HW * TAIL_HW / 4;
    const int b = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int nb = min(max(p.nb, JOINT_MIN_BINS), JOINT_MAX_BINS);
    const int rh = min(min(max(p.hradius, 0), TRACK_MAX_R), (nb - 1) / 2);
    float4* A = reinterpret_cast<float4*>(jr_smem);                    // [nb][64] the slices' c at this group's cells, then g there
    float* mw = reinterpret_cast<float*>(A + nb * JS_QUADS);           // [2 rh + 2] merged weights, mw[d + rh] = M[d]
    // o, f and M[d]: track_joint_mix_kernel's statements
    const double u0 = -((double)p.turn_deg[b] / (360.0 / (double)nb));
    const double fl0 = floor(u0);
    const float f = (float)(u0 - fl0);
    int o = (int)fmin(fmax(fl0, -1073741824.), 1073741824.) % nb;
    if (o < 0) o += nb;
    if (tid < 2 * rh + 2) {
        const int d = tid - rh;
        const int a = d < 0 ? -d : d, c = d - 1 < 0 ? 1 - d : d - 1;   // |d|, |d - 1|
        const float* th = p.htaps + (size_t)b * p.htaps_stride;
        const float ta = a <= rh ? th[a] : 0.f, tc = c <= rh ? th[c] : 0.f;
        mw[tid] = fmaf(f, tc, (1.f - f) * ta);
    }
    const size_t base = (size_t)b * nb * n4 + (size_t)g * JS_QUADS + lane;
    const float4* src = reinterpret_cast<const float4*>(p.work) + base;
    for (int k = wave; k < nb; k += 4) A[k * JS_QUADS + lane] = src[(size_t)k * n4];
    __syncthreads();
    const float fl = p.floor[b];
    const float4* nxt = reinterpret_cast<const float4*>(p.next) + base;
    double acc[1] = {0.0};
    // a thread's bins wave, wave + 4, ..: g stays in registers (every index a constant of the unrolled loop) until the whole workgroup
    // has formed its priors, then takes A's place in LDS
    float4 q[JS_BINS_PER_WAVE];
#pragma unroll
    for (int i = 0; i < JS_BINS_PER_WAVE; ++i) {
        const int k = wave + 4 * i;
        q[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < nb) {
            const float4 sn = nxt[(size_t)k * n4];
            int j = k + o - rh;                                        // in (-nb, 2 nb): the first source bin, on the circle
            if (j < 0) j += nb;
            if (j >= nb) j -= nb;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int d = 0; d <= 2 * rh + 1; ++d) {
                const float4 v = A[j * JS_QUADS + lane];
                const float w = mw[d];
                a.x = fmaf(w, v.x, a.x); a.y = fmaf(w, v.y, a.y); a.z = fmaf(w, v.z, a.z); a.w = fmaf(w, v.w, a.w);
                if (++j == nb) j = 0;
            }
            q[i].x = sn.x > 0.f ? sn.x / (a.x + fl) : 0.f;
            q[i].y = sn.y > 0.f ? sn.y / (a.y + fl) : 0.f;
            q[i].z = sn.z > 0.f ? sn.z / (a.z + fl) : 0.f;
            q[i].w = sn.w > 0.f ? sn.w / (a.w + fl) : 0.f;
            acc[0] += (double)q[i].x; acc[0] += (double)q[i].y; acc[0] += (double)q[i].z; acc[0] += (double)q[i].w;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < JS_BINS_PER_WAVE; ++i) {
        const int k = wave + 4 * i;
        if (k < nb) A[k * JS_QUADS + lane] = q[i];
    }
    __syncthreads();
    // the adjoint of the mix: g(k) went to k' = (k + o + d) mod nb with M[d], so h(k') gathers g((k' - o - d) mod nb), d ascending
    float4* dst = reinterpret_cast<float4*>(p.work) + base;
    for (int k = wave; k < nb; k += 4) {
        int j = k - o + rh;                                            // in (-nb, 2 nb): the source bin of d = -rh
        if (j < 0) j += nb;
        if (j >= nb) j -= nb;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int d = 0; d <= 2 * rh + 1; ++d) {
            const float4 v = A[j * JS_QUADS + lane];
            const float w = mw[d];
            a.x = fmaf(w, v.x, a.x); a.y = fmaf(w, v.y, a.y); a.z = fmaf(w, v.z, a.z); a.w = fmaf(w, v.w, a.w);
            if (--j < 0) j = nb - 1;
        }
        dst[(size_t)k * n4] = a;
    }
    summ_wave_to_lds<1>(acc, red);
    __syncthreads();
    if (tid == 0) {
        summ_from_lds<1>(acc, red);
        joint_smooth_work(p.work, p.B, nb).gpart[(size_t)b * JS_GROUPS + g] = acc[0];
    }
}

__global__ __launch_bounds__(256) void track_joint_smooth_weight_kernel(const TrackJointSmoothParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char jw_smem[];
    __shared__ double red[4], redG;
    constexpr int HW = TAIL_HW, n = HW * HW;
    const int s = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;      // slice s = b * nb + k'
    const int r = p.radius;
    const int nb = min(max(p.nb, JOINT_MIN_BINS), JOINT_MAX_BINS);
    const int b = s / nb, k = s - b * nb;
    const int Y0 = (t / (HW / TRACK_T)) * TRACK_T, X0 = (t % (HW / TRACK_T)) * TRACK_T;
    const TrackTile tile = track_tile(jw_smem, r);
    const JointSmoothWork wk = joint_smooth_work(p.work, p.B, nb);
    if (tid < 64) {
        const double G = joint_smooth_sum_groups(wk.gpart + (size_t)b * JS_GROUPS);
        if (tid == 0) redG = G;
    }
    // h[k'] is one more [512][512] map: slice s is map 0 of the batch at work + s * n, with its own shift and its query's taps
    track_stage_shifted(tile, p.work + (size_t)s * n, p.shift + (size_t)s * 2, -1.f, p.taps + (size_t)b * p.taps_stride, 0, 0, r, Y0, X0);
    __syncthreads();
    const float4 c = track_blur_passes<1>(tile.src, tile.S, tile.P, tile.mid, tile.wx, tile.wy, r);
    const int cell = (Y0 + (tid >> 3)) * HW + X0 + (tid & 7) * 4;
    const double G = redG;
    const float fl = p.floor[b], Gf = (float)G;
    const bool keep = G == 0.0;     // the next joint has no positive value and says nothing; the result is J itself
    const float4 J = *reinterpret_cast<const float4*>(p.joint + (size_t)s * n + cell);
    float4 w;
    w.x = keep ? J.x : J.x * fmaf(fl, Gf, c.x);
    w.y = keep ? J.y : J.y * fmaf(fl, Gf, c.y);
    w.z = keep ? J.z : J.z * fmaf(fl, Gf, c.z);
    w.w = keep ? J.w : J.w * fmaf(fl, Gf, c.w);
    *reinterpret_cast<float4*>(p.smoothed + (size_t)s * n + cell) = w;
    double acc[1] = {0.0};
    acc[0] += (double)w.x; acc[0] += (double)w.y; acc[0] += (double)w.z; acc[0] += (double)w.w;
    summ_wave_to_lds<1>(acc, red);
    __syncthreads();
    if (tid == 0) {
        summ_from_lds<1>(acc, red);
        wk.wpart[((size_t)b * JOINT_MAX_BINS + k) * TRACK_TILES + t] = acc[0];
    }
}

__global__ __launch_bounds__(256) void track_joint_smooth_scale_kernel(const TrackJointSmoothParams p) {
    __shared__ double zr[4], gsh;
    __shared__ double hw[JOINT_MAX_BINS][4];
    __shared__ float sv[4];
    __shared__ int si[4];
    constexpr int n = TAIL_HW * TAIL_HW;
    const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x;
    const int nb = min(max(p.nb, JOINT_MIN_BINS), JOINT_MAX_BINS);
    const int lo = ch * (n / TAIL_CHUNKS);
    const JointSmoothWork wk = joint_smooth_work(p.work, p.B, nb);
    if (tid < 64) {
        const double G = joint_smooth_sum_groups(wk.gpart + (size_t)b * JS_GROUPS);
        if (tid == 0) gsh = G;
    }
    double z[1] = {0.0};
    for (int k = 0; k < nb; ++k) z[0] += wk.wpart[((size_t)b * JOINT_MAX_BINS + k) * TRACK_TILES + tid];
    summ_wave_to_lds<1>(z, zr);
    __syncthreads();
    const double Z = ((zr[0] + zr[1]) + zr[2]) + zr[3], G = gsh;
    const float inv = (float)(1.0 / Z);
    const bool keep = G == 0.0;                        // `smoothed` already holds J
    const bool good = joint_smooth_good(Z);            // else: no smoothed joint, all zero
    float4 mg[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) mg[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 q[4], qn[4];
    load_chunk<false>(p.smoothed + (size_t)b * nb * n, nullptr, lo, q);
    for (int k = 0; k < nb; ++k) {
        load_chunk<false>(p.smoothed + ((size_t)b * nb + min(k + 1, nb - 1)) * n, nullptr, lo, qn);
        float4* dst = reinterpret_cast<float4*>(p.smoothed + ((size_t)b * nb + k) * n + lo);
        double h[1] = {0.0};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float4 S = keep ? q[u] : good ? make_float4(q[u].x * inv, q[u].y * inv, q[u].z * inv, q[u].w * inv) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (!keep) dst[tid + u * 256] = S;
            mg[u].x += S.x; mg[u].y += S.y; mg[u].z += S.z; mg[u].w += S.w;
            h[0] += (double)S.x; h[0] += (double)S.y; h[0] += (double)S.z; h[0] += (double)S.w;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = qn[u];
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
        // the next address reuses this store's registers at once: two wait states behind the 16-byte store, as in kernels_track_joint.hip
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
        float* pair = wk.pairs + ((size_t)b * TAIL_CHUNKS + ch) * 2;
        pair[0] = best;
        pair[1] = __int_as_float(bi);
        if (ch == 0) { wk.zg[(size_t)b * 2] = Z; wk.zg[(size_t)b * 2 + 1] = G; }
    }
    if (tid < nb) wk.hpart[((size_t)b * JOINT_MAX_BINS + tid) * TAIL_CHUNKS + ch] = ((hw[tid][0] + hw[tid][1]) + hw[tid][2]) + hw[tid][3];
}

// Grid (B), 256 threads: wave v totals the bins v, v + 4, ..; the first wave the marginal's argmax and, with it, the row
__global__ __launch_bounds__(256) void track_joint_smooth_finish_kernel(const TrackJointSmoothParams p) {
    constexpr int n = TAIL_HW * TAIL_HW;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int nb = min(max(p.nb, JOINT_MIN_BINS), JOINT_MAX_BINS);
    const JointSmoothWork wk = joint_smooth_work(p.work, p.B, nb);
    for (int k = wave; k < nb; k += 4) {
        const double v = joint_smooth_sum_chunks(wk.hpart + ((size_t)b * JOINT_MAX_BINS + k) * TAIL_CHUNKS);
        if (lane == 0) p.hist[(size_t)b * nb + k] = (float)v;
    }
    if (tid < 64) {
        const float* pr = wk.pairs + ((size_t)b * TAIL_CHUNKS + lane) * 2;
        float best = pr[0];
        int bi = __float_as_int(pr[1]);
        argmax_wave(best, bi);
        if (tid == 0) {
            const double Z = wk.zg[(size_t)b * 2], G = wk.zg[(size_t)b * 2 + 1];
            const bool keep = G == 0.0;
            // a value is taken when it is above -inf; a marginal without one has no argmax
            const bool has = (keep || joint_smooth_good(Z)) && best > -INFINITY && (unsigned)bi < (unsigned)n;
            float* row = p.stats + (size_t)b * JOINT_SMOOTH_COLS;
            int bk = -1;
            if (has) {
                float bv = -INFINITY;
                for (int k = 0; k < nb; ++k) {
                    const float v = p.smoothed[((size_t)b * nb + k) * n + bi];
                    if (v > bv) { bv = v; bk = k; }          // (the first of equal values)
                }
            }
            row[0] = has ? (float)bi : -1.f;
            row[1] = has ? best : NAN;
            row[2] = (float)bk;
            row[3] = keep ? NAN : (float)Z;
            row[4] = (float)G;
        }
    }
}

static size_t joint_smooth_ratio_lds_bytes(int nb, int rh) { return sizeof(float4) * (size_t)nb * JS_QUADS + sizeof(float) * (2 * rh + 2); }

void launch_track_joint_smooth(const TrackJointSmoothParams& p, hipStream_t s) {
    TrackJointPredictParams xy{};
    xy.joint = p.joint; xy.shift = p.shift; xy.taps = p.taps; xy.taps_stride = p.taps_stride; xy.radius = p.radius; xy.work = p.work;
    xy.B = p.B; xy.nb = p.nb;
    launch_track_joint_xy(xy, s);
    const size_t lds = track_lds_bytes(p.radius), ratio_lds = joint_smooth_ratio_lds_bytes(p.nb, p.hradius);
    static LdsAttr ratio_attr, weight_attr;
    ensure_dynamic_lds(ratio_attr, reinterpret_cast<const void*>(track_joint_smooth_ratio_kernel), ratio_lds);
    ensure_dynamic_lds(weight_attr, reinterpret_cast<const void*>(track_joint_smooth_weight_kernel), lds);
    CCVPE_LAUNCH(track_joint_smooth_ratio_kernel, dim3(JS_GROUPS, p.B), dim3(256), ratio_lds, s, p);
    CCVPE_LAUNCH(track_joint_smooth_weight_kernel, dim3(TRACK_TILES, p.B * p.nb), dim3(256), lds, s, p);
    CCVPE_LAUNCH(track_joint_smooth_scale_kernel, dim3(TAIL_CHUNKS, p.B), dim3(256), 0, s, p);
    CCVPE_LAUNCH(track_joint_smooth_finish_kernel, dim3(p.B), dim3(256), 0, s, p);
}

}  // namespace ccvpe
