// Heading posterior (the outputs are defined in kernels.h): the position posterior of a pose plan, folded over the
// orientation field into a histogram of headings and circular moments.  Reference: the heading of a pose is the (cos, sin) lookup and
// acos-sign rule at the argmax pixel (train_VIGOR.py:297-311); this applies that rule to every pixel, weighted with the heatmap.
#include "kernels.h"
#include "tail_shared.h"

namespace ccvpe {

static constexpr int HD_SUMS = 3;                   // M, sum h c, sum h s
static_assert(HD_SUMS <= HEADING_PART, "hand-off row");
#ifndef CCVPE_HEADING_WAVE_COMBINE
#define CCVPE_HEADING_WAVE_COMBINE 1   // dev builds (tools/build_variant.sh): 0 = every lane adds for itself, what the combined path is timed against
#endif

// h at a cell with the field (c, s) into a[0 .. 3): an invalid cell adds 0.  h * c is exact in float64 (24 x 24 bits): every add rounds once
__device__ __forceinline__ void heading_take(double (&a)[HD_SUMS], float h, float c, float s, bool valid) {
    const double hd = valid ? (double)h : 0.0;
    a[0] += hd;
    a[1] += hd * (double)(valid ? c : 0.f);
    a[2] += hd * (double)(valid ? s : 0.f);
}

// mean direction of (S, C) in degrees [0, 360); NaN when the resultant length is zero (or not a number)
__device__ __forceinline__ float heading_mean_deg(double S, double C, double R) {
    if (!(R > 0.0)) return NAN;
    double d = atan2(S, C) * 57.295779513082320877;
    if (d < 0.0) d += 360.0;
    const float f = (float)d;
    return f >= 360.f ? 0.f : f;
}

// Grid (64 chunks, B), 256 threads: chunk c of sample b is pose_argmax_kernel's chunk c, read the same way (four float4 of logits, of
// the prior, and two times four float4 of the field per thread, all in flight in one trip), its values recomputed as that kernel's
// (posterior_value) from softmax_stats' (m, inv): the bits of the posterior map.
// Histogram: q = (unsigned long long)(h * 2^52) - an exact scaling (h <= 1) and one truncation - added as 64-bit integers into the
// workgroup's LDS histogram, then into the query's bins[] with agent-scope integer adds (non-empty bins only).  Integer sums have no
// order, so the bits do not depend on who arrives when.  The orientation field is smooth: the 64 cells a wave handles at once mostly
// share a bin, and 64 lanes adding to one LDS word serialise - a wave whose lanes agree sums q with xor shuffles and one lane adds.
// M, sum h c, sum h s: float64, thread -> xor shuffles -> four waves in LDS -> agent-scope hand-off -> the last arriver, lane = chunk.
// Last arriver (ticket.h): swaps every bin of the query for zero (the read and the reset in one operation at the memory side),
// converts, finds the mode, runs the window pass around the argmax with all its threads, and thread 0 writes the twelve columns.
// Every global address lies inside its tensor: whole chunks, bins below nbins <= HEADING_MAX_BINS (clamped), a window clipped to the
// grid around a clamped index, lanes past the window re-reading that index and adding 0.
template <bool PRIOR>
__global__ __launch_bounds__(256) void heading_reduce_kernel(const HeadingParams p) {
    __shared__ float gm, gs;
    __shared__ unsigned flag;
    __shared__ unsigned long long lh[HEADING_MAX_BINS];
    __shared__ float lf[HEADING_MAX_BINS];
    __shared__ double sd[4 * HD_SUMS];
    constexpr int n = TAIL_HW * TAIL_HW, per = n / TAIL_CHUNKS;   // 4096: a multiple of 4 x 256
    const int b = blockIdx.y, c = blockIdx.x, lo = c * per;
    const int nb = min(max(p.nbins, HEADING_MIN_BINS), HEADING_MAX_BINS);
    softmax_stats(p.partial, b, TAIL_CHUNKS, gm, gs);
    for (int i = threadIdx.x; i < nb; i += 256) lh[i] = 0ull;
    const float* lg = p.logits + (size_t)b * n;
    const float* lp = PRIOR ? p.prior + (size_t)b * p.prior_stride : nullptr;
    const float* oc = p.ori + (size_t)b * 2 * n;
    const float* os = oc + n;
    float4 v[4], fc[4], fs[4];
    load_chunk<PRIOR>(lg, lp, lo, v);
#pragma unroll
    for (int u = 0; u < 4; ++u) fc[u] = reinterpret_cast<const float4*>(oc + lo)[threadIdx.x + u * 256];
#pragma unroll
    for (int u = 0; u < 4; ++u) fs[u] = reinterpret_cast<const float4*>(os + lo)[threadIdx.x + u * 256];
    __syncthreads();
    const float m = gm, inv = gs;
    const bool ok = isfinite(m) && isfinite(inv);     // (else the sample has no posterior: nothing is added anywhere)
    const float scale = (float)nb / 360.f;
    double acc[HD_SUMS] = {0.0, 0.0, 0.0};
    auto cell = [&](float x, float cs, float sn) {
        const float h = posterior_value(x, m, inv);    // pose_argmax_kernel's take()
        const bool valid = ok && heading_valid(cs, sn);
        heading_take(acc, h, cs, sn, valid);
        int bin = heading_bin(cs, sn, scale, nb);     // (tail_shared.h)
        bin = valid ? bin : -1;
        const unsigned long long q = valid && h > 0.f ? (unsigned long long)(h * 4503599627370496.f) : 0ull;
        if (CCVPE_HEADING_WAVE_COMBINE && __all(bin == __builtin_amdgcn_readfirstlane(bin))) {   // one bin for the wave: one add
            unsigned long long t = q;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
            if ((threadIdx.x & 63) == 0 && bin >= 0 && t) atomicAdd(&lh[bin], t);
        } else if (q) {
            atomicAdd(&lh[bin], q);
        }
    };
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        cell(v[u].x, fc[u].x, fs[u].x); cell(v[u].y, fc[u].y, fs[u].y); cell(v[u].z, fc[u].z, fs[u].z); cell(v[u].w, fc[u].w, fs[u].w);
    }
    summ_wave_to_lds(acc, sd);
    __syncthreads();
    if (threadIdx.x == 0) {
        summ_from_lds(acc, sd);
#pragma unroll
        for (int k = 0; k < HD_SUMS; ++k) st_sc1(p.part + ((size_t)b * TAIL_CHUNKS + c) * HEADING_PART + k, acc[k]);
    }
    unsigned long long* bins = p.bins + (size_t)b * HEADING_MAX_BINS;
    for (int i = threadIdx.x; i < nb; i += 256) {
        const unsigned long long t = lh[i];
        if (t) (void)__hip_atomic_fetch_add(bins + i, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!ticket_arrive(p.tickets + b, 1u, (unsigned)TAIL_CHUNKS, &flag)) return;

    // ---- last arriver of sample b ----
    double g[HD_SUMS] = {0.0, 0.0, 0.0};
    sums_from_chunks(p.part + (size_t)b * TAIL_CHUNKS * HEADING_PART, HEADING_PART, g);
    for (int i = threadIdx.x; i < nb; i += 256) {
        const unsigned long long t = __hip_atomic_exchange(bins + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float hf = (float)((double)t * 2.220446049250313e-16);   // 2^-52: a total below 2^53 is exact in float64
        p.hist[(size_t)b * nb + i] = hf;
        lf[i] = hf;
    }
    const int r = min(max(p.r, 0), HEADING_MAX_R);
    const int bi = ok ? min(max(p.index[b], 0), n - 1) : 0;
    const Window win = window_around(bi, r);
    const int cells = win.cells;
    double w[HD_SUMS] = {0.0, 0.0, 0.0};
    for (int i0 = threadIdx.x; i0 < cells; i0 += 256 * WINDOW_UB) {
        float hv[WINDOW_UB], cv[WINDOW_UB], sv[WINDOW_UB];
#pragma unroll
        for (int u = 0; u < WINDOW_UB; ++u) {
            const int at = win.at(i0 + u * 256, bi);
            float x = lg[at];
            if constexpr (PRIOR) x += lp[at];
            hv[u] = posterior_value(x, m, inv);
            cv[u] = oc[at];
            sv[u] = os[at];
        }
#pragma unroll
        for (int u = 0; u < WINDOW_UB; ++u) heading_take(w, hv[u], cv[u], sv[u], ok && i0 + u * 256 < cells && heading_valid(cv[u], sv[u]));
    }
    summ_wave_to_lds(w, sd);
    __syncthreads();                                  // (lf[] is complete as well)
    if (threadIdx.x >= 64) return;
    float bv = -1.f;
    int bm = 0x7fffffff;
    for (int i = threadIdx.x; i < nb; i += 64) { const float t = lf[i]; if (t > bv) { bv = t; bm = i; } }   // strictly greater keeps the first
    argmax_wave(bv, bm);
    if (threadIdx.x != 0) return;
    summ_from_lds(w, sd);
    float* row = p.heading + (size_t)b * HEADING_COLS;
    const float nan = NAN;
    if (!ok) {
#pragma unroll
        for (int k = 0; k < HEADING_COLS; ++k) row[k] = k == 5 ? -1.f : nan;
        return;
    }
    const double M = g[0], C = g[1] / M, S = g[2] / M, R = sqrt(C * C + S * S);
    row[0] = (float)M; row[1] = (float)C; row[2] = (float)S; row[3] = heading_mean_deg(S, C, R); row[4] = (float)R;
    row[5] = (float)bm; row[6] = (float)((double)bv / M);
    const double Mw = w[0], Cw = w[1] / Mw, Sw = w[2] / Mw, Rw = sqrt(Cw * Cw + Sw * Sw);
    row[7] = (float)Mw; row[8] = (float)Cw; row[9] = (float)Sw; row[10] = heading_mean_deg(Sw, Cw, Rw); row[11] = (float)Rw;
}

void launch_heading_reduce(const HeadingParams& p, hipStream_t s) {
    if (p.prior) CCVPE_LAUNCH(heading_reduce_kernel<true>, dim3(TAIL_CHUNKS, p.B), dim3(256), 0, s, p);
    else CCVPE_LAUNCH(heading_reduce_kernel<false>, dim3(TAIL_CHUNKS, p.B), dim3(256), 0, s, p);
}

}  // namespace ccvpe
