// Output-side kernels: the last 3x3 conv of each decoder (16 -> 1 logits, 16 -> 2 orientation with the
// unit normalisation fused), the 262144-way softmax, the test-loop post-processing and a layout helper.
//
// Reference: conv1[2] / conv1_ori[2] (models.py:423-425, 444-446), flatten + Softmax(dim=-1)
// (models.py:628-629), F.normalize(x_ori, p=2, dim=1) (models.py:650), argmax / (cos,sin) lookup /
// acos-sign rule (train_VIGOR.py:297-311).
#include "kernels.h"
#include "tail_shared.h"

#include <algorithm>

namespace ccvpe {

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// thread = one output pixel; 9 taps x 16 channels = 4 float4 per tap, NHWC input (64 B per pixel).
template <int COUT>
__global__ __launch_bounds__(256) void tail_conv_kernel(const TailConvParams p) {
    __shared__ float ws[9 * 16 * COUT];
    for (int i = threadIdx.x; i < 9 * 16 * COUT; i += 256) ws[i] = p.w[i];
    __syncthreads();
    const long long total = (long long)p.B * p.H * p.W;
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= total) return;
    const int x = (int)(pix % p.W);
    const long long t = pix / p.W;
    const int y = (int)(t % p.H);
    const int b = (int)(t / p.H);
    float acc[COUT];
#pragma unroll
    for (int o = 0; o < COUT; ++o) acc[o] = p.bias[o];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = y + ky - 1;
        if ((unsigned)iy >= (unsigned)p.H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = x + kx - 1;
            if ((unsigned)ix >= (unsigned)p.W) continue;
            const float* src = p.in + (((size_t)b * p.H + iy) * p.W + ix) * 16;
            const float* w = ws + (ky * 3 + kx) * 16 * COUT;
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                const float4 v = *reinterpret_cast<const float4*>(src + c4 * 4);
#pragma unroll
                for (int o = 0; o < COUT; ++o) {
                    acc[o] = fmaf(v.x, w[(c4 * 4 + 0) * COUT + o], acc[o]);
                    acc[o] = fmaf(v.y, w[(c4 * 4 + 1) * COUT + o], acc[o]);
                    acc[o] = fmaf(v.z, w[(c4 * 4 + 2) * COUT + o], acc[o]);
                    acc[o] = fmaf(v.w, w[(c4 * 4 + 3) * COUT + o], acc[o]);
                }
            }
        }
    }
    const size_t hw = (size_t)p.H * p.W;
    const size_t opix = (size_t)y * p.W + x;
    if (p.raw) {
#pragma unroll
        for (int o = 0; o < COUT; ++o) p.raw[((size_t)b * COUT + o) * hw + opix] = acc[o];
    }
    if (p.normalize) {
        float n2 = 0.f;
#pragma unroll
        for (int o = 0; o < COUT; ++o) n2 = fmaf(acc[o], acc[o], n2);
        const float inv = 1.f / fmaxf(sqrtf(n2), 1e-12f);
#pragma unroll
        for (int o = 0; o < COUT; ++o) acc[o] *= inv;
    }
#pragma unroll
    for (int o = 0; o < COUT; ++o) p.out[((size_t)b * COUT + o) * hw + opix] = acc[o];
}

void launch_tail_conv(const TailConvParams& p, hipStream_t s) {
    long long total = (long long)p.B * p.H * p.W;
    int blocks = (int)((total + 255) / 256);
    if (p.cout == 1) CCVPE_LAUNCH(tail_conv_kernel<1>, dim3(blocks), dim3(256), 0, s, p);
    else CCVPE_LAUNCH(tail_conv_kernel<2>, dim3(blocks), dim3(256), 0, s, p);
}

// ------------------------------------------------------------------------------------------------
// Softmax over n = 262144 logits per sample, two launches: per-chunk online (max, sum exp) partials,
// then every block re-derives the sample's (max, sum) from the partials and normalises its chunk.
// ------------------------------------------------------------------------------------------------
// (combine(), softmax_stats() and posterior_value(): tail_shared.h)

// PRIOR: the partials of l' = fl32(l + prior), the prior read as float4 beside the logits; everything else - and so
// every bit for a zero prior - as without it.  A prior excludes pixels with -inf, often whole stretches: a thread that has seen
// nothing else keeps (-inf, 0) instead of exp(-inf - -inf) = NaN, as combine() does.
template <bool PRIOR>
__global__ __launch_bounds__(256) void softmax_partial_kernel(const SoftmaxParams p) {
    __shared__ float sm[4], ss[4];
    const int b = blockIdx.y, ch = blockIdx.x;
    const int per = p.n / p.chunks;
    const float4* src = reinterpret_cast<const float4*>(p.logits + (size_t)b * p.n + (size_t)ch * per);
    const float4* lp = PRIOR ? reinterpret_cast<const float4*>(p.prior + (size_t)b * p.prior_stride + (size_t)ch * per) : nullptr;
    float m = -INFINITY, s = 0.f;
    for (int i = threadIdx.x; i < per / 4; i += 256) {
        float4 v = src[i];
        if constexpr (PRIOR) { const float4 q = lp[i]; v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w; }
        const float lm = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
        const float mn = fmaxf(m, lm);
        if constexpr (PRIOR) { if (mn == -INFINITY) continue; }
        s = s * __expf(m - mn) + __expf(v.x - mn) + __expf(v.y - mn) + __expf(v.z - mn) + __expf(v.w - mn);
        m = mn;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float m2 = __shfl_xor(m, off), s2 = __shfl_xor(s, off);
        combine(m, s, m2, s2);
    }
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6] = m; ss[threadIdx.x >> 6] = s; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) combine(m, s, sm[w], ss[w]);
        p.partial[((size_t)b * p.chunks + ch) * 2 + 0] = m;
        p.partial[((size_t)b * p.chunks + ch) * 2 + 1] = s;
    }
}

__global__ __launch_bounds__(256) void softmax_final_kernel(const SoftmaxParams p) {
    __shared__ float gm, gs;
    const int b = blockIdx.y, ch = blockIdx.x;
    softmax_stats(p.partial, b, p.chunks, gm, gs);
    __syncthreads();
    const float m = gm, inv = gs;
    const int per = p.n / p.chunks;
    const float4* src = reinterpret_cast<const float4*>(p.logits + (size_t)b * p.n + (size_t)ch * per);
    float4* dst = reinterpret_cast<float4*>(p.out + (size_t)b * p.n + (size_t)ch * per);
    for (int i = threadIdx.x; i < per / 4; i += 256) {
        const float4 v = src[i];
        dst[i] = make_float4(posterior_value(v.x, m, inv), posterior_value(v.y, m, inv), posterior_value(v.z, m, inv), posterior_value(v.w, m, inv));
    }
}

void launch_softmax(const SoftmaxParams& p, hipStream_t s) {
    CCVPE_LAUNCH(softmax_partial_kernel<false>, dim3(p.chunks, p.B), dim3(256), 0, s, p);
    CCVPE_LAUNCH(softmax_final_kernel, dim3(p.chunks, p.B), dim3(256), 0, s, p);
}

void launch_softmax_partial(const SoftmaxParams& p, hipStream_t s) {
    if (p.prior) CCVPE_LAUNCH(softmax_partial_kernel<true>, dim3(p.chunks, p.B), dim3(256), 0, s, p);
    else CCVPE_LAUNCH(softmax_partial_kernel<false>, dim3(p.chunks, p.B), dim3(256), 0, s, p);
}

// ------------------------------------------------------------------------------------------------
// Post-processing: argmax (first maximal index, as numpy.argmax on a map without NaN; NaN never wins: DESIGN.md 2.3), prob, (cos, sin),
// angle in degrees.
// ------------------------------------------------------------------------------------------------
// Round 4: one workgroup per sample scanned its 262144 values in sixteen rounds of loads - 16 trips to memory for ONE workgroup at batch 1
// (17 us).  Now TAIL_CHUNKS workgroups per sample take 4096 values each (all their loads in one trip), leave (max, first index) per chunk
// and draw a ticket (ticket.h); the workgroup that draws a sample's last one reduces the TAIL_CHUNKS pairs - the maximum with the
// first-index tie-break does not depend on the order - and writes the pose.  `rows` != null: the same five numbers as floats
// ([B][5]: index, prob, cos, sin, angle - the rows the data-parallel gather moves) instead of the ccvpe_pose records.
__global__ __launch_bounds__(256) void postprocess_kernel(const float* heat, const float* ori, int n, PoseOut* out, float* rows, float* part, unsigned* tickets) {
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ unsigned flag;
    const int b = blockIdx.y, c = blockIdx.x;
    const float* h = heat + (size_t)b * n;
    const int lo = (int)((long long)n * c / TAIL_CHUNKS) & ~3, hi = c + 1 == TAIL_CHUNKS ? n : (int)((long long)n * (c + 1) / TAIL_CHUNKS) & ~3;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    auto take = [&](float v, int i) { if (v > best) { best = v; bi = i; } };   // strictly greater keeps the first index per thread
    if ((reinterpret_cast<uintptr_t>(h) & 15) == 0) {
        const float4* h4 = reinterpret_cast<const float4*>(h);
        const int q_lo = lo >> 2, q_hi = hi >> 2;
        for (int i = q_lo + threadIdx.x; i < q_hi; i += 4 * 256) {   // four independent 16-byte loads in flight per round (one round at 512 x 512)
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = i + u * 256 < q_hi ? h4[i + u * 256] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = (i + u * 256) * 4;
                take(v[u].x, e); take(v[u].y, e + 1); take(v[u].z, e + 2); take(v[u].w, e + 3);
            }
        }
        for (int j = (q_hi << 2) + threadIdx.x; j < hi; j += 256) take(h[j], j);
    } else {
        for (int j = lo + threadIdx.x; j < hi; j += 256) take(h[j], j);
    }
    argmax_wave(best, bi);
    argmax_publish(best, bi, sv, si, part + ((size_t)b * TAIL_CHUNKS + c) * 2);
    if (!ticket_arrive(tickets + b, 1u, (unsigned)TAIL_CHUNKS, &flag)) return;
    if (threadIdx.x < 64) {
        argmax_from_pairs(part + (size_t)b * TAIL_CHUNKS * 2, best, bi);
        if (threadIdx.x == 0) {
            // no value above -inf anywhere (all NaN, all -inf, a mix): nothing was taken and bi is still the sentinel.  The sample has no
            // posterior: index -1, prob NaN, the orientation of pixel 0.  The clamp keeps the reads inside ori regardless.
            const bool ok = bi != 0x7fffffff;
            const int at = ok ? min(max(bi, 0), n - 1) : 0;
            const float cs = ori[((size_t)b * 2 + 0) * n + at];
            const float sn = ori[((size_t)b * 2 + 1) * n + at];
            const float ang = pose_angle_deg(cs, sn);
            if (!ok) { bi = -1; best = NAN; }
            if (rows) {
                rows[b * 5 + 0] = (float)bi; rows[b * 5 + 1] = best; rows[b * 5 + 2] = cs; rows[b * 5 + 3] = sn; rows[b * 5 + 4] = ang;
            } else {
                out[b].index = bi;
                out[b].prob = best;
                out[b].cos_v = cs;
                out[b].sin_v = sn;
                out[b].angle_deg = ang;
            }
        }
    }
}

// scratch = [PP_MAX_BATCH ticket counters][B x TAIL_CHUNKS (max, index) pairs]; the counters are zero before the first launch and every launch
// leaves them at zero (a larger buffer serves a smaller batch: the counters do not move)
size_t postprocess_scratch_bytes(int B) { return ((size_t)PP_MAX_BATCH + (size_t)B * TAIL_CHUNKS * 2) * sizeof(float); }

void launch_postprocess(const float* heat, const float* ori, int B, int n, PoseOut* out, float* rows, void* scratch, hipStream_t s) {
    unsigned* tickets = reinterpret_cast<unsigned*>(scratch);
    float* part = reinterpret_cast<float*>(scratch) + PP_MAX_BATCH;
    CCVPE_LAUNCH(postprocess_kernel, dim3(TAIL_CHUNKS, B), dim3(256), 0, s, heat, ori, n, out, rows, part, tickets);
}

// ------------------------------------------------------------------------------------------------
// Posterior summary (the row is defined in kernels.h): the accumulation and reduction steps pose_argmax_kernel<.., SUMM>
// (values recomputed from the logits) and belief_summary_kernel (a stored map) share, so that the two forms are one definition.
// Seven float64 sums per map - S0, Sx, Sy, Sxx, Sxy, Syy, S(h ln h) - over the 64 chunk workgroups: every thread adds its values, the
// wave reduces with xor shuffles, the four waves meet in LDS (wave order), thread 0 hands the chunk's sums to the sample's last
// arriver (ticket.h) beside the (max, index) pair.  The last arriver adds the 64 chunks' sums (lane = chunk, then the xor shuffles),
// runs the window pass around the argmax with all its threads (six sums of at most 65 x 65 values, reduced the same way) and thread 0
// writes the row.  Every order is fixed: the same map gives the same bits whoever arrives last.
// ------------------------------------------------------------------------------------------------
static constexpr int SM_SUMS = 7, SM_WIN = 6;       // sums per map, per window (no entropy term)
static_assert(SM_SUMS <= SUMMARY_PART && TAIL_CHUNKS == 64, "one lane of the last arriver's first wave per chunk");

// h at index i into a[0 .. n): S0, Sx, Sy, Sxx, Sxy, Syy and, n == 7, S(h ln h) (h == 0 adds 0).  h * x and h * y are exact in float64,
// h * x * x below 2^42 as well: every fused multiply-add rounds once, like the add alone
template <int n>
__device__ __forceinline__ void summ_take(double (&a)[n], float h, int i) {
    const double hd = (double)h, x = (double)(i & (TAIL_HW - 1)), y = (double)(i >> 9);
    const double hx = hd * x, hy = hd * y;
    a[0] += hd; a[1] += hx; a[2] += hy;
    a[3] = fma(hx, x, a[3]); a[4] = fma(hx, y, a[4]); a[5] = fma(hy, y, a[5]);
    if constexpr (n > SM_WIN) a[6] = fma(hd, h > 0.f ? (double)logf(h) : 0.0, a[6]);
}

// (summ_wave_to_lds() and summ_from_lds(), the wave and workgroup steps: tail_shared.h)
// thread 0 of chunk c: the chunk's sums to the hand-off (agent-scope stores, before ticket_arrive)
__device__ __forceinline__ void summ_publish(const double (&a)[SM_SUMS], double* part) {
#pragma unroll
    for (int k = 0; k < SM_SUMS; ++k) st_sc1(part + k, a[k]);
}

// All 256 threads of a sample's last arriver, behind ticket_arrive and a barrier that made (bi, best) uniform.  part: the sample's
// [64][SUMMARY_PART] hand-off; h_at(i): the map's value at index i in [0, 512 * 512), the expression the sums were taken of; lds:
// 4 * SM_SUMS doubles nobody else touches; ok: the sample has a posterior (else the row is (-1, NaN, NaN ...)).  The window loads
// go out WINDOW_UB per thread at a time.
template <class HAt>
__device__ __forceinline__ void summ_finish(const double* part, int bi, float best, bool ok, int r, HAt h_at, double* lds, float* row) {
    double g[SM_SUMS];
    sums_from_chunks(part, SUMMARY_PART, g);
    const Window win = window_around(bi, r);
    const int cells = win.cells;
    double w[SM_WIN] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i0 = threadIdx.x; i0 < cells; i0 += 256 * WINDOW_UB) {
        float hv[WINDOW_UB];
        int at[WINDOW_UB];
#pragma unroll
        for (int u = 0; u < WINDOW_UB; ++u) {
            at[u] = win.at(i0 + u * 256, bi);
            hv[u] = h_at(at[u]);
        }
#pragma unroll
        for (int u = 0; u < WINDOW_UB; ++u) summ_take(w, i0 + u * 256 < cells ? hv[u] : 0.f, at[u]);
    }
    summ_wave_to_lds(w, lds);
    __syncthreads();
    if (threadIdx.x != 0) return;
    summ_from_lds(w, lds);
    const float nan = NAN;
    row[0] = ok ? (float)bi : -1.f;
    row[1] = ok ? best : nan;
    const double S0 = g[0], W0 = w[0];
    row[2] = ok ? (float)S0 : nan;
    if (!ok || S0 == 0.0) {
#pragma unroll
        for (int k = 3; k < SUMMARY_COLS; ++k) row[k] = nan;
        return;
    }
    const double mx = g[1] / S0, my = g[2] / S0, wx = w[1] / W0, wy = w[2] / W0;
    row[3] = (float)(log(S0) - g[6] / S0);
    row[4] = (float)mx; row[5] = (float)my;
    row[6] = (float)(g[3] / S0 - mx * mx); row[7] = (float)(g[4] / S0 - mx * my); row[8] = (float)(g[5] / S0 - my * my);
    row[9] = (float)(W0 / S0);
    row[10] = (float)wx; row[11] = (float)wy;
    row[12] = (float)(w[3] / W0 - wx * wx); row[13] = (float)(w[4] / W0 - wx * wy); row[14] = (float)(w[5] / W0 - wy * wy);
    row[15] = (float)cells;
}

// ------------------------------------------------------------------------------------------------
// Pose plans (ccvpe_localize): postprocess_kernel's argmax over a heatmap that is never stored.  Chunk c of sample b is postprocess_kernel's
// chunk c (4096 values); its values are recomputed from the logits by posterior_value (tail_shared.h) with softmax_final_kernel's (m, inv), i.e. the
// bits that kernel would store, so index and prob are those ccvpe_postprocess_rows reads from the heatmap, ties included (strictly greater
// within a thread, lowest index on ties across threads and chunks).  Every thread's index starts at the first position it scans, so the
// result is a position of the chunk whatever the values are.
// PRIOR: the values are those of l' = fl32(l + prior), with softmax_partial_kernel<true>'s statistics.  A sample whose
// (m, inv) is not finite (a prior of -inf everywhere, a +inf, a NaN) has no posterior: rows (-1, NaN) and index 0, so that the
// orientation launches behind still read inside the map.
// POST (ccvpe_track_update*): the values the chunk has just recomputed are also stored, as float4, to posterior[b] - the
// map softmax_final_kernel would store for l'.  Every workgroup knows (m, inv), so each applies the rule for a sample without a finite
// posterior to its own chunk: all zeros.
// SUMM (ccvpe_*_summary): the summary row of that map, from the values in registers - the chunk's seven float64 sums go
// to the last arriver beside its (max, index) pair, and the last arriver, the argmax in hand, recomputes the window around it with
// posterior_value (summ_finish).  A sample without a finite posterior: (-1, NaN, NaN ...), with or without a prior.
// ------------------------------------------------------------------------------------------------
template <bool PRIOR, bool POST = false, bool SUMM = false>
__global__ __launch_bounds__(256) void pose_argmax_kernel(const PoseArgmaxParams p) {
    __shared__ float gm, gs;
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ unsigned flag;
    __shared__ double sd[SUMM ? 4 * SM_SUMS : 1];
    double acc[SM_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int b = blockIdx.y, c = blockIdx.x;
    softmax_stats(p.partial, b, p.chunks, gm, gs);
    const int per = p.n / p.chunks;                   // 4096: a multiple of 4 x 256
    const int lo = c * per;
    const float* lg = p.logits + (size_t)b * p.n;
    const float* lp = PRIOR ? p.prior + (size_t)b * p.prior_stride : nullptr;
    float4 v[4];
    load_chunk<PRIOR>(lg, lp, lo, v);                 // (per / 4 = 1024 float4 per chunk: four per thread, one trip)
    __syncthreads();
    const float m = gm, inv = gs;
    if (p.stats && c == 0 && threadIdx.x == 0) { p.stats[b * 2 + 0] = m; p.stats[b * 2 + 1] = inv; }   // (read by a later launch)
    float best = -INFINITY;
    int bi = lo + 4 * (int)threadIdx.x;
    auto take = [&](float x, int i) { const float h = posterior_value(x, m, inv); if (h > best) { best = h; bi = i; } };
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int e = lo + (threadIdx.x + u * 256) * 4;
        take(v[u].x, e); take(v[u].y, e + 1); take(v[u].z, e + 2); take(v[u].w, e + 3);
    }
    if constexpr (POST) {
        float4* dst = reinterpret_cast<float4*>(p.posterior + (size_t)b * p.n + lo);
        const bool fin = isfinite(m) && isfinite(inv);
        // SUMM: the same 16 bytes through a buffer descriptor over the chunk.  Beside the float64 sums the scheduler fills the slot
        // behind a global 16-byte store with the next store's address computation, on the address registers of the first - harmless,
        // but tests/test_isa_hazard.py reads a store's first operand as its data; a buffer store names its data first.
        const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(dst, 0, SUMM ? per * (int)sizeof(float) : 0, 0x00020000);
#pragma unroll
        for (int u = 0; u < 4; ++u) {   // take()'s values: the bits rows[b][1] carries at the argmax
            const float4 h = make_float4(posterior_value(v[u].x, m, inv), posterior_value(v[u].y, m, inv), posterior_value(v[u].z, m, inv),
                                         posterior_value(v[u].w, m, inv));
            if constexpr (SUMM) {
                const tk_f32x4 o = fin ? tk_f32x4{h.x, h.y, h.z, h.w} : tk_f32x4{0.f, 0.f, 0.f, 0.f};
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(tk_u32x4, o), prs, (threadIdx.x + u * 256) * 16u, 0, 0);
            } else {
                dst[threadIdx.x + u * 256] = fin ? h : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    }
    if constexpr (SUMM) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {   // take()'s values again: the values of the map
            const int e = lo + (threadIdx.x + u * 256) * 4;
            summ_take(acc, posterior_value(v[u].x, m, inv), e); summ_take(acc, posterior_value(v[u].y, m, inv), e + 1);
            summ_take(acc, posterior_value(v[u].z, m, inv), e + 2); summ_take(acc, posterior_value(v[u].w, m, inv), e + 3);
        }
        summ_wave_to_lds(acc, sd);
    }
    argmax_wave(best, bi);
    argmax_publish(best, bi, sv, si, p.pairs + ((size_t)b * p.chunks + c) * 2);
    if constexpr (SUMM) {
        if (threadIdx.x == 0) {
            summ_from_lds(acc, sd);
            summ_publish(acc, p.summ_part + ((size_t)b * p.chunks + c) * SUMMARY_PART);
        }
    }
    if (!ticket_arrive(p.tickets + b, 1u, (unsigned)p.chunks, &flag)) return;
    if (threadIdx.x < 64) {
        argmax_from_pairs(p.pairs + (size_t)b * p.chunks * 2, best, bi);
        if constexpr (SUMM) {
            if (threadIdx.x == 0) { sv[0] = best; si[0] = bi; }
        } else if (threadIdx.x == 0) {
            // (every form: without a prior the map softmax_final_kernel would store is then all NaN, which postprocess_kernel answers alike)
            if (!(isfinite(m) && isfinite(inv))) { p.index[b] = 0; p.rows[b * 5 + 0] = -1.f; p.rows[b * 5 + 1] = NAN; return; }
            p.index[b] = bi;
            p.rows[b * 5 + 0] = (float)bi;
            p.rows[b * 5 + 1] = best;
        }
    }
    if constexpr (SUMM) {
        __syncthreads();
        const bool ok = isfinite(m) && isfinite(inv);
        best = sv[0]; bi = ok ? min(max(si[0], 0), p.n - 1) : 0;   // (a position of the map by construction; the clamp keeps the window reads inside it regardless)
        if (threadIdx.x == 0) {
            p.index[b] = bi;
            p.rows[b * 5 + 0] = ok ? (float)bi : -1.f;
            p.rows[b * 5 + 1] = ok ? best : NAN;
        }
        auto h_at = [&](int i) {
            float x = lg[i];
            if constexpr (PRIOR) x += lp[i];
            return posterior_value(x, m, inv);
        };
        summ_finish(p.summ_part + (size_t)b * p.chunks * SUMMARY_PART, bi, best, ok, p.summary_r, h_at, sd, p.summary + (size_t)b * SUMMARY_COLS);
    }
}

void launch_pose_argmax(const PoseArgmaxParams& p, hipStream_t s) {
    if (p.summary) {
        if (p.posterior && p.prior) CCVPE_LAUNCH((pose_argmax_kernel<true, true, true>), dim3(p.chunks, p.B), dim3(256), 0, s, p);
        else if (p.posterior) CCVPE_LAUNCH((pose_argmax_kernel<false, true, true>), dim3(p.chunks, p.B), dim3(256), 0, s, p);
        else if (p.prior) CCVPE_LAUNCH((pose_argmax_kernel<true, false, true>), dim3(p.chunks, p.B), dim3(256), 0, s, p);
        else CCVPE_LAUNCH((pose_argmax_kernel<false, false, true>), dim3(p.chunks, p.B), dim3(256), 0, s, p);
        return;
    }
    if (p.posterior && p.prior) CCVPE_LAUNCH((pose_argmax_kernel<true, true>), dim3(p.chunks, p.B), dim3(256), 0, s, p);
    else if (p.posterior) CCVPE_LAUNCH((pose_argmax_kernel<false, true>), dim3(p.chunks, p.B), dim3(256), 0, s, p);
    else if (p.prior) CCVPE_LAUNCH(pose_argmax_kernel<true>, dim3(p.chunks, p.B), dim3(256), 0, s, p);
    else CCVPE_LAUNCH(pose_argmax_kernel<false>, dim3(p.chunks, p.B), dim3(256), 0, s, p);
}

// The summary of a stored map (ccvpe_belief_summary): postprocess_kernel's chunks (4096 values per workgroup, four float4 per thread in
// one trip; a map that is not 16-byte aligned is read value by value) with pose_argmax_kernel's rules for the index - every thread
// starts at the first position it scans, strictly greater within a thread, lowest index across threads and chunks, so NaN never wins
// and the index is a position of the map whatever it holds - and the sums, hand-off and last arriver of the SUMM form.
__global__ __launch_bounds__(256) void belief_summary_kernel(const BeliefSummaryParams p) {
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ unsigned flag;
    __shared__ double sd[4 * SM_SUMS];
    constexpr int n = TAIL_HW * TAIL_HW, per = n / TAIL_CHUNKS;   // 4096: a multiple of 4 x 256
    const int b = blockIdx.y, c = blockIdx.x, lo = c * per;
    const float* h = p.belief + (size_t)b * n;
    double acc[SM_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    float best = -INFINITY;
    int bi;
    auto take = [&](float v, int i) { if (v > best) { best = v; bi = i; } summ_take(acc, v, i); };
    if ((reinterpret_cast<uintptr_t>(h) & 15) == 0) {
        const float4* h4 = reinterpret_cast<const float4*>(h + lo);
        bi = lo + 4 * (int)threadIdx.x;
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = h4[threadIdx.x + u * 256];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = lo + (threadIdx.x + u * 256) * 4;
            take(v[u].x, e); take(v[u].y, e + 1); take(v[u].z, e + 2); take(v[u].w, e + 3);
        }
    } else {
        bi = lo + (int)threadIdx.x;
        float v[per / 256];
#pragma unroll
        for (int u = 0; u < per / 256; ++u) v[u] = h[lo + threadIdx.x + u * 256];
#pragma unroll
        for (int u = 0; u < per / 256; ++u) take(v[u], lo + threadIdx.x + u * 256);
    }
    summ_wave_to_lds(acc, sd);
    argmax_wave(best, bi);
    argmax_publish(best, bi, sv, si, p.pairs + ((size_t)b * TAIL_CHUNKS + c) * 2);
    if (threadIdx.x == 0) {
        summ_from_lds(acc, sd);
        summ_publish(acc, p.summ_part + ((size_t)b * TAIL_CHUNKS + c) * SUMMARY_PART);
    }
    if (!ticket_arrive(p.tickets + b, 1u, (unsigned)TAIL_CHUNKS, &flag)) return;
    if (threadIdx.x < 64) {
        argmax_from_pairs(p.pairs + (size_t)b * TAIL_CHUNKS * 2, best, bi);
        if (threadIdx.x == 0) { sv[0] = best; si[0] = bi; }
    }
    __syncthreads();
    best = sv[0];
    bi = min(max(si[0], 0), n - 1);   // (a position of the map by construction; the clamp keeps the window reads inside it regardless)
    if (best == -INFINITY) best = h[bi];   // nothing was taken (no value above -inf): column 1 is the map's value at the index, like any other row's
    summ_finish(p.summ_part + (size_t)b * TAIL_CHUNKS * SUMMARY_PART, bi, best, true, p.r, [&](int i) { return h[i]; }, sd,
                p.summary + (size_t)b * SUMMARY_COLS);
}

void launch_belief_summary(const BeliefSummaryParams& p, hipStream_t s) {
    CCVPE_LAUNCH(belief_summary_kernel, dim3(TAIL_CHUNKS, p.B), dim3(256), 0, s, p);
}

// ------------------------------------------------------------------------------------------------
// Cross-tile reduction of ccvpe_localize_region: one wave per query over its pairs offsets[g] .. offsets[g+1]-1, in
// float64.  S_p = exp(m_p - M) / inv_p is pair p's unnormalised mass (m_p, inv_p: pose_argmax_kernel's statistics, M the query's largest
// finite m_p; 0 for a pair whose statistics are not finite), Z = sum S_p, tile_prob[p] = S_p / Z, joint_p = prob_p * S_p / Z.  The best
// pair is the first with the largest joint_p (NaN never wins; none at all: the first pair, whose probability is then NaN).  Indices are
// only copied from pair_rows, never dereferenced.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void region_reduce_kernel(const RegionParams p) {
    const int g = blockIdx.x;
    const int lo = p.off[g], hi = p.off[g + 1];
    const int t = threadIdx.x;
    auto finite = [&](int q) { return isfinite(p.stats[q * 2 + 0]) && isfinite(p.stats[q * 2 + 1]); };
    double M = -INFINITY;
    for (int q = lo + t; q < hi; q += 64)
        if (finite(q)) M = fmax(M, (double)p.stats[q * 2 + 0]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) M = fmax(M, __shfl_xor(M, o));
    auto mass = [&](int q) { return finite(q) ? exp((double)p.stats[q * 2 + 0] - M) / (double)p.stats[q * 2 + 1] : 0.0; };
    double Z = 0.0;
    for (int q = lo + t; q < hi; q += 64) Z += mass(q);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) Z += __shfl_xor(Z, o);
    double bv = 0.0;
    int bq = -1;   // eligible pair with the largest joint probability, lowest position on ties
    for (int q = lo + t; q < hi; q += 64) {
        const double S = mass(q);
        p.tile_prob[q] = (float)(S / Z);
        const double j = (double)p.pair_rows[q * 5 + 1] * S / Z;
        if (finite(q) && j == j && (bq < 0 || j > bv)) { bv = j; bq = q; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double v2 = __shfl_xor(bv, o);
        const int q2 = __shfl_xor(bq, o);
        if (q2 >= 0 && (bq < 0 || v2 > bv || (v2 == bv && q2 < bq))) { bv = v2; bq = q2; }
    }
    if (t == 0) {
        const int q = bq >= 0 ? bq : lo;
        const float* r = p.pair_rows + (size_t)q * 5;
        float* o = p.rows + (size_t)(p.g0 + g) * 5;
        o[0] = r[0];
        o[1] = bq >= 0 ? (float)bv : NAN;
        o[2] = r[2]; o[3] = r[3]; o[4] = r[4];
        p.best_pair[p.g0 + g] = q;
    }
}

void launch_region_reduce(const float* stats, const float* pair_rows, const int* offsets, int G, float* rows, int* best_pair, float* tile_prob,
                          hipStream_t s) {
    for (int g0 = 0; g0 < G; g0 += REGION_MAX_QUERIES) {
        RegionParams p{};
        p.stats = stats; p.pair_rows = pair_rows; p.rows = rows; p.best_pair = best_pair; p.tile_prob = tile_prob; p.g0 = g0;
        const int n = std::min(REGION_MAX_QUERIES, G - g0);
        for (int k = 0; k <= n; ++k) p.off[k] = offsets[g0 + k];
        CCVPE_LAUNCH(region_reduce_kernel, dim3(n), dim3(64), 0, s, p);
    }
}

__global__ __launch_bounds__(64) void pose_gather_kernel(const float* ori, const int* index, int B, int n, float* rows) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int i = min(max(index[b], 0), n - 1);
    const float cs = ori[((size_t)b * 2 + 0) * n + i];
    const float sn = ori[((size_t)b * 2 + 1) * n + i];
    rows[b * 5 + 2] = cs;
    rows[b * 5 + 3] = sn;
    rows[b * 5 + 4] = pose_angle_deg(cs, sn);
}

void launch_pose_gather(const float* ori, const int* index, int B, int n, float* rows, hipStream_t s) {
    CCVPE_LAUNCH(pose_gather_kernel, dim3((B + 63) / 64), dim3(64), 0, s, ori, index, B, n, rows);
}

// ------------------------------------------------------------------------------------------------
// Top-K peaks (ccvpe_postprocess_topk, ccvpe_localize_topk): pixel q suppresses p when q != p lies in p's (2r+1)^2 window and
// (H[q], -q) > (H[p], -p); p is a peak when H[p] > 0 and nothing suppresses it.  A pixel's key is u(p) = bits of H[p] when H[p] > 0
// (positive floats order like their bit patterns), else 0 - so NaN, zeros and pixels outside the image never suppress anything -
// and p is a peak iff u(p) > 0 and p is the raster-first maximum of u over its window.  That maximum is separable: the first maximum
// of each row segment (strictly greater keeps the leftmost), then the first of those down the column (strictly greater keeps the
// topmost row, and a higher row holds the lower index whatever its column).
//
// Grid (64 tiles, B): a workgroup owns a 64 x 64 tile, stages the tile plus an r halo as keys in LDS (from the stored heatmap, or
// recomputed from the logits with softmax_final_kernel's (m, inv) and expression - the same bits), finds its peaks, sorts them as
// 64-bit keys (value bits << 32 | ~index: value descending, index ascending) with a bitonic sort in LDS and hands its best K to the
// sample's last arriver (ticket.h), which sorts the 64 K candidates the same way and writes index[b][k] and rows[b][k][0..1].  A slot
// without a peak gets index -1 and the row (-1, 0, 0, 0, 0); the orientation launches behind skip it.
// PRIOR (logits path only): the values are posterior_value(l + prior) with softmax_partial_kernel<true>'s statistics;
// a sample whose (m, inv) is not finite has no peak at all.
// ------------------------------------------------------------------------------------------------
static constexpr int TK_T = 64;                    // tile side
static constexpr int TK_TILES = (TAIL_HW / TK_T) * (TAIL_HW / TK_T);   // 64 per sample
static_assert(TK_T * TK_T * (4 + 5) >= TK_TILES * TOPK_MAX_K * 8, "the sort buffer aliases the smallest staging area");

__host__ __device__ constexpr int topk_halo(int r) { return TK_T + 2 * r; }
// staging: keys [S][S], row maxima [S][64] and their column offsets [S][64] (bytes); the sort buffer (<= 4096 keys) aliases them
static size_t topk_lds_bytes(int r) { const size_t S = topk_halo(r); return (S * S * 4 + S * TK_T * 5 + 7) & ~(size_t)7; }

// descending bitonic sort of s[0, N), N a power of two >= 2; every thread of the workgroup calls it, and it ends at a barrier
__device__ __forceinline__ void topk_sort_desc(unsigned long long* s, int N) {
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int q = threadIdx.x; q < N / 2; q += 256) {
                const int i = 2 * q - (q & (j - 1)), l = i + j;
                const unsigned long long a = s[i], c = s[l];
                if ((i & k) == 0 ? a < c : a > c) { s[i] = c; s[l] = a; }
            }
            __syncthreads();
        }
}

template <bool LOGITS, bool PRIOR = false>
__global__ __launch_bounds__(256) void topk_peaks_kernel(const TopkParams p) {
    static_assert(LOGITS || !PRIOR, "the prior applies to recomputed values");
    extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
    __shared__ float gm, gs;
    __shared__ unsigned cnt, flag;
    constexpr int HW = TAIL_HW, n = HW * HW;
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const int r = p.r, S = topk_halo(r);
    const int Y0 = (t / (HW / TK_T)) * TK_T, X0 = (t % (HW / TK_T)) * TK_T;
    unsigned* in = reinterpret_cast<unsigned*>(tk_smem);                    // [S][S]
    unsigned* hv = in + S * S;                                              // [S][64]
    unsigned char* hc = reinterpret_cast<unsigned char*>(hv + S * TK_T);   // [S][64]
    unsigned long long* sk = reinterpret_cast<unsigned long long*>(tk_smem);
    float m = 0.f, inv = 0.f;
    if (LOGITS) {
        softmax_stats(p.partial, b, TAIL_CHUNKS, gm, gs);   // (the chunks of the pose plans' softmax.partial launch)
        __syncthreads();
        m = gm; inv = gs;
    }
    if (tid == 0) cnt = 0u;
    const float* src = (LOGITS ? p.logits : p.heat) + (size_t)b * n;
    const float* lpb = PRIOR ? p.prior + (size_t)b * p.prior_stride : nullptr;
    const bool finite_stats = !PRIOR || (isfinite(m) && isfinite(inv));
    for (int i = tid; i < S * S; i += 256) {
        const int ly = i / S, lx = i - ly * S;
        const int y = Y0 - r + ly, x = X0 - r + lx;
        unsigned u = 0u;
        if ((unsigned)y < (unsigned)HW && (unsigned)x < (unsigned)HW) {
            float h = src[y * HW + x];
            if constexpr (PRIOR) h = posterior_value(h + lpb[y * HW + x], m, inv);
            else if (LOGITS) h = posterior_value(h, m, inv);
            u = h > 0.f && finite_stats ? __float_as_uint(h) : 0u;
        }
        in[i] = u;
    }
    __syncthreads();
    // first maximum of every row segment [x - r, x + r] of the S staged rows
    for (int i = tid; i < S * TK_T; i += 256) {
        const unsigned* row = in + (i >> 6) * S + (i & 63);
        unsigned best = row[0];
        int bc = 0;
#pragma unroll 8
        for (int d = 1; d <= 2 * r; ++d) { const unsigned v = row[d]; if (v > best) { best = v; bc = d; } }   // (8 LDS reads in flight)
        hv[i] = best;
        hc[i] = (unsigned char)bc;
    }
    __syncthreads();
    // the 16 pixels of this thread: peak test, then its key (0: no peak)
    unsigned long long key[TK_T * TK_T / 256];
#pragma unroll
    for (int u = 0; u < TK_T * TK_T / 256; ++u) {
        const int j = tid + u * 256, py = j >> 6, px = j & 63;
        const unsigned mine = in[(py + r) * S + px + r];
        const int own = (py + r) * TK_T + px;
        bool peak = mine != 0u && hv[own] == mine && hc[own] == r;   // (p is the first maximum of its own row segment)
        if (peak) {
            const unsigned* col = hv + py * TK_T + px;
            unsigned best = col[0];
            int br = 0;
#pragma unroll 8
            for (int d = 1; d <= 2 * r; ++d) { const unsigned v = col[d * TK_T]; if (v > best) { best = v; br = d; } }
            peak = br == r;
        }
        const unsigned idx = (unsigned)((Y0 + py) * HW + X0 + px);
        key[u] = peak ? ((unsigned long long)mine << 32) | (unsigned long long)(~idx) : 0ull;
    }
    __syncthreads();   // the staging area becomes the sort buffer
#pragma unroll
    for (int u = 0; u < TK_T * TK_T / 256; ++u)
        if (key[u]) sk[atomicAdd(&cnt, 1u)] = key[u];
    __syncthreads();
    const int np = (int)cnt;
    int N = TOPK_MAX_K;
    while (N < np) N <<= 1;
    for (int i = np + tid; i < N; i += 256) sk[i] = 0ull;
    __syncthreads();
    topk_sort_desc(sk, N);
    const int K = p.k;
    unsigned long long* hand = p.keys + ((size_t)b * TK_TILES + t) * K;
    for (int i = tid; i < K; i += 256) __hip_atomic_store(hand + i, sk[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!ticket_arrive(p.tickets + b, 1u, (unsigned)TK_TILES, &flag)) return;
    // last arriver of sample b: the best K of the 64 K candidates
    const int M = TK_TILES * K;
    N = TOPK_MAX_K;
    while (N < M) N <<= 1;
    const unsigned long long* all = p.keys + (size_t)b * TK_TILES * K;
    for (int i = tid; i < N; i += 256) sk[i] = i < M ? __hip_atomic_load(all + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    __syncthreads();
    topk_sort_desc(sk, N);
    for (int i = tid; i < K; i += 256) {
        const unsigned long long kv = sk[i];
        float* row = p.rows + ((size_t)b * K + i) * 5;
        if (kv) {
            const int idx = (int)~(unsigned)kv;
            p.index[b * K + i] = idx;
            row[0] = (float)idx;
            row[1] = __uint_as_float((unsigned)(kv >> 32));
        } else {
            p.index[b * K + i] = -1;
            row[0] = -1.f; row[1] = 0.f; row[2] = 0.f; row[3] = 0.f; row[4] = 0.f;
        }
    }
}

void launch_topk_peaks(const TopkParams& p, hipStream_t s) {
    const size_t lds = topk_lds_bytes(p.r);
    if (p.logits && p.prior) {
        static LdsAttr attr;
        ensure_dynamic_lds(attr, reinterpret_cast<const void*>(topk_peaks_kernel<true, true>), lds);
        CCVPE_LAUNCH((topk_peaks_kernel<true, true>), dim3(TK_TILES, p.B), dim3(256), lds, s, p);
    } else if (p.logits) {
        static LdsAttr attr;
        ensure_dynamic_lds(attr, reinterpret_cast<const void*>(topk_peaks_kernel<true>), lds);
        CCVPE_LAUNCH(topk_peaks_kernel<true>, dim3(TK_TILES, p.B), dim3(256), lds, s, p);
    } else {
        static LdsAttr attr;
        ensure_dynamic_lds(attr, reinterpret_cast<const void*>(topk_peaks_kernel<false>), lds);
        CCVPE_LAUNCH(topk_peaks_kernel<false>, dim3(TK_TILES, p.B), dim3(256), lds, s, p);
    }
}

// pose_gather_kernel for K hypotheses per sample: thread = slot (b, k); slots without a peak (index -1) keep their row
__global__ __launch_bounds__(64) void topk_gather_kernel(const float* ori, const int* index, int B, int K, int n, float* rows) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= B * K) return;
    const int i = index[t];
    if (i < 0 || i >= n) return;
    const int b = t / K;
    const float cs = ori[((size_t)b * 2 + 0) * n + i];
    const float sn = ori[((size_t)b * 2 + 1) * n + i];
    rows[(size_t)t * 5 + 2] = cs;
    rows[(size_t)t * 5 + 3] = sn;
    rows[(size_t)t * 5 + 4] = pose_angle_deg(cs, sn);
}

void launch_topk_gather(const float* ori, const int* index, int B, int K, int n, float* rows, hipStream_t s) {
    CCVPE_LAUNCH(topk_gather_kernel, dim3((B * K + 63) / 64), dim3(64), 0, s, ori, index, B, K, n, rows);
}

size_t topk_scratch_bytes(int B) {
    return (size_t)PP_MAX_BATCH * sizeof(unsigned) + (size_t)B * TK_TILES * TOPK_MAX_K * sizeof(unsigned long long) +
           (size_t)B * TOPK_MAX_K * sizeof(int);
}

// ------------------------------------------------------------------------------------------------
// GT-side test-loop metrics (second half): train_VIGOR.py:296-326, train_KITTI.py:309-343.  One thread per
// query, double precision like the reference's numpy / math code.  Inputs: the pose of postprocess_kernel, the heatmap (for
// the probability at the ground-truth pixel) and per-query ground truth from the dataset side.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double angle_deg_of(double c, double s) {   // math.acos + the sign rule of train_VIGOR.py:307-311
    const double a = acos(c) * 57.29577951308232;                       // math.degrees
    if (s < 0.0) { double m = fmod(-a, 360.0); if (m < 0.0) m += 360.0; return m; }   // Python's % 360
    return a;
}

__global__ __launch_bounds__(64) void metrics_kernel(const PoseOut* pose, const float* heat, int B, int W, int n, const int* gt_index,
                                                     const float* gt_cos_sin, const double* meter_per_pixel, const double* heading_deg,
                                                     MetricsOut* out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int pi = pose[b].index, gi = gt_index[b];
    const int py = pi / W, px = pi - py * W, gy = gi / W, gx = gi - gy * W;
    const double dy = (double)(gy - py), dx = (double)(gx - px);
    MetricsOut m;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    m.pixel_distance = pi < 0 ? nan : sqrt(dy * dy + dx * dx);   // (index -1: the sample has no posterior, DESIGN.md 2.3 - NaN distances)
    m.meter_distance = m.pixel_distance * meter_per_pixel[b];
    m.prob_at_gt = (unsigned)gi < (unsigned)n ? (double)heat[(size_t)b * n + gi] : nan;   // (a ground truth outside the map: no read)
    const double cp = (double)pose[b].cos_v, sp = (double)pose[b].sin_v;
    m.angle_pred_deg = m.angle_gt_deg = m.orientation_error_deg = nan;
    if (fabs(cp) <= 1.0 && fabs(sp) <= 1.0) {    // the reference skips the orientation error otherwise (train_VIGOR.py:306)
        m.angle_pred_deg = angle_deg_of(cp, sp);
        if (gt_cos_sin) {
            m.angle_gt_deg = angle_deg_of((double)gt_cos_sin[2 * b], (double)gt_cos_sin[2 * b + 1]);
            const double d = fabs(m.angle_gt_deg - m.angle_pred_deg);
            m.orientation_error_deg = fmin(d, 360.0 - d);
        }
    }
    m.longitudinal_m = m.lateral_m = nan;
    if (heading_deg) {                            // train_KITTI.py:318-325
        const double gt2pred = atan2(fabs(dx), fabs(dy)) * 180.0 / 3.141592653589793;
        const double diff = fabs(heading_deg[b] - gt2pred);
        m.longitudinal_m = fabs(cos(diff * 3.141592653589793 / 180.0) * m.pixel_distance) * meter_per_pixel[b];
        m.lateral_m = fabs(sin(diff * 3.141592653589793 / 180.0) * m.pixel_distance) * meter_per_pixel[b];
    }
    out[b] = m;
}

void launch_metrics(const PoseOut* pose, const float* heat, int B, int W, int n, const int* gt_index, const float* gt_cos_sin,
                    const double* meter_per_pixel, const double* heading_deg, MetricsOut* out, hipStream_t s) {
    CCVPE_LAUNCH(metrics_kernel, dim3((B + 63) / 64), dim3(64), 0, s, pose, heat, B, W, n, gt_index, gt_cos_sin, meter_per_pixel, heading_deg, out);
}

// ------------------------------------------------------------------------------------------------
// Input pre-processing: uint8 HWC image (already decoded / resized on the host) ->
// ToTensor (x/255) -> Normalize((x-mean)/std) (train_VIGOR.py:57-70) -> panorama roll
// torch.roll(grd, shift, dims=2) (datasets.py:118) -> FoV width crop grd[..., :crop_w]
// (train_VIGOR.py:272-273), written as the fp32 NCHW tensor forward() consumes.  Same fp32 operation
// order as torchvision (divide, subtract, divide), so results are bit-identical.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void preprocess_kernel(const PreprocParams p) {
    const long long total = (long long)p.B * 3 * p.H * p.crop_w;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int x = (int)(i % p.crop_w);
        long long t = i / p.crop_w;
        const int y = (int)(t % p.H);
        t /= p.H;
        const int c = (int)(t % 3);
        const int b = (int)(t / 3);
        int sx = x - (p.shift ? p.shift[b] : 0);
        sx %= p.W;
        if (sx < 0) sx += p.W;
        const float v = (float)p.in[(((size_t)b * p.H + y) * p.W + sx) * 3 + c];
        p.out[i] = (v / 255.0f - p.mean[c]) / p.stdv[c];
    }
}

void launch_preprocess(const PreprocParams& p, hipStream_t s) {
    const long long total = (long long)p.B * 3 * p.H * p.crop_w;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 256 * 32) blocks = 256 * 32;
    CCVPE_LAUNCH(preprocess_kernel, dim3(blocks), dim3(256), 0, s, p);
}

__device__ __forceinline__ void put4(const Dst& d, long long pix, int c, float4 v) {
    const size_t e = (size_t)pix * d.ld + d.coff + c;
    if (d.split) {   // bf16x3 mode: two bf16 planes
        typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
        const float f[4] = {v.x, v.y, v.z, v.w};
        bf16x4_t h, l;
#pragma unroll
        for (int k = 0; k < 4; ++k) { h[k] = (__bf16)f[k]; l[k] = (__bf16)(f[k] - (float)h[k]); }
        __bf16* hp = reinterpret_cast<__bf16*>(d.ptr);
        *reinterpret_cast<bf16x4_t*>(hp + e) = h;
        *reinterpret_cast<bf16x4_t*>(hp + d.plane + e) = l;
    } else {
        *reinterpret_cast<float4*>(d.ptr + e) = v;
    }
}

// contiguous [P][C] -> channel window of an NHWC buffer (cached aerial taps -> decoder concat buffers)
__global__ __launch_bounds__(256) void scatter_channels_kernel(const float* src, int C, long long P, Dst d0, Dst d1, int ndst) {
    const int c4n = C >> 2;
    const long long total = P * c4n;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long pix = i / c4n;
        const int c4 = (int)(i - pix * c4n);
        const float4 v = *reinterpret_cast<const float4*>(src + pix * C + c4 * 4);
        put4(d0, pix, c4 * 4, v);
        if (ndst > 1) put4(d1, pix, c4 * 4, v);
    }
}

void launch_scatter_channels(const float* src, int C, long long P, Dst d0, Dst d1, int ndst, hipStream_t s) {
    const long long total = P * (C >> 2);
    int blocks = (int)((total + 255) / 256);
    if (blocks > 256 * 16) blocks = 256 * 16;
    CCVPE_LAUNCH(scatter_channels_kernel, dim3(blocks), dim3(256), 0, s, src, C, P, d0, d1, ndst);
}

// [n_tiles][hw][C] -> channel window of an NHWC buffer, destination sample b0 + blockIdx.y reading source sample tile[blockIdx.y]
// (indexed cached forms: several queries share one cached aerial tile).  The source sample is uniform per block, so its index is
// one scalar load from the launch arguments.  Samples that share a tile re-read the same lines, which mostly hit L2 / MALL.
__global__ __launch_bounds__(256) void gather_channels_kernel(const GatherParams p) {
    const int c4n = p.C >> 2;
    const unsigned n = (unsigned)p.hw * (unsigned)c4n;   // float4 per sample (<= 2^18)
    const int b = blockIdx.y;
    const float4* __restrict__ src = reinterpret_cast<const float4*>(p.src + (size_t)p.tile[b] * p.hw * p.C);
    const long long pix0 = (long long)(p.b0 + b) * p.hw;
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const unsigned q = i / (unsigned)c4n;
        const int c = (int)(i - q * (unsigned)c4n) * 4;
        const float4 v = src[i];   // [hw][C] contiguous: float4 i is pixel q, channels c..c+3
        put4(p.d0, pix0 + q, c, v);
        if (p.ndst > 1) put4(p.d1, pix0 + q, c, v);
    }
}

void launch_gather_channels(const float* src, int C, int hw, const int* tile, int B, Dst d0, Dst d1, int ndst, hipStream_t s) {
    const unsigned n = (unsigned)hw * (unsigned)(C >> 2);
    for (int b0 = 0; b0 < B; b0 += GATHER_MAX_SAMPLES) {
        GatherParams p{};
        p.src = src; p.d0 = d0; p.d1 = d1; p.ndst = ndst; p.C = C; p.hw = hw; p.b0 = b0;
        const int nb = std::min(GATHER_MAX_SAMPLES, B - b0);
        for (int k = 0; k < nb; ++k) p.tile[k] = tile[b0 + k];
        // about as many blocks in flight as the scatter it replaces (4096 at most)
        const int per = (int)std::max<unsigned>(1, std::min<unsigned>((n + 255) / 256, 256u * 16 / nb));
        CCVPE_LAUNCH(gather_channels_kernel, dim3(per, nb), dim3(256), 0, s, p);
    }
}

// NHWC view -> NCHW copy (debug taps only).
__global__ void nhwc_to_nchw_kernel(const float* in, int in_ld, int coff, int C, int B, int HW, float* out) {
    const long long total = (long long)B * C * HW;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int p = (int)(i % HW);
        const long long t = i / HW;
        const int c = (int)(t % C);
        const int b = (int)(t / C);
        out[i] = in[((size_t)b * HW + p) * in_ld + coff + c];
    }
}

// Unit-variance pseudo-random floats (sum of three uniforms on [-1, 1): the autotuner's operands - timing candidates on
// zeros ranks them at a clock the real data never sees).  Counter-based (PCG hash of the element index): any grid gives the same bits.
__global__ __launch_bounds__(256) void fill_random_kernel(float* __restrict__ p, size_t n, uint32_t seed) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float acc = 0.f;
        uint32_t st = (uint32_t)i * 747796405u + (uint32_t)(i >> 32) * 2891336453u + seed;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            st = st * 747796405u + 2891336453u;
            uint32_t w = ((st >> ((st >> 28u) + 4u)) ^ st) * 277803737u;
            w = (w >> 22u) ^ w;
            acc += (float)(w >> 8) * (2.0f / 16777216.0f) - 1.0f;
        }
        p[i] = acc;
    }
}
__global__ __launch_bounds__(256) void multi_copy_kernel(const MultiCopy mc) {
    // blockIdx.y = segment; 16-byte pieces, grid-stride
    const int seg = blockIdx.y;
    const unsigned long long n4 = mc.n[seg] >> 2;
    const f32x4_t* __restrict__ src = reinterpret_cast<const f32x4_t*>(mc.src[seg]);
    f32x4_t* __restrict__ dst = reinterpret_cast<f32x4_t*>(mc.dst[seg]);
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (unsigned long long)gridDim.x * 256) dst[i] = src[i];
}
void launch_multi_copy(const MultiCopy& mc, hipStream_t s) {
    if (mc.count <= 0) return;
    unsigned long long mx = 0;
    for (int i = 0; i < mc.count; ++i) mx = std::max(mx, mc.n[i]);
    const int gx = (int)std::min<unsigned long long>((mx / 4 + 255) / 256, 512);
    CCVPE_LAUNCH(multi_copy_kernel, dim3(std::max(gx, 1), mc.count), dim3(256), 0, s, mc);
}

void launch_fill_random(float* p, size_t n, uint32_t seed, hipStream_t s) {
    if (n == 0) return;
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 256 * 32);
    CCVPE_LAUNCH(fill_random_kernel, dim3(blocks), dim3(256), 0, s, p, n, seed);
}

void launch_nhwc_to_nchw(const float* in, int in_ld, int coff, int C, int B, int HW, float* out, hipStream_t s) {
    long long total = (long long)B * C * HW;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 65535) blocks = 65535;
    CCVPE_LAUNCH(nhwc_to_nchw_kernel, dim3(blocks), dim3(256), 0, s, in, in_ld, coff, C, B, HW, out);
}

}  // namespace ccvpe
