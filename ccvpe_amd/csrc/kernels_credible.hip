// Credible regions (the outputs are defined in include/ccvpe.h and kernels.h): per query the smallest union of whole
// value classes of the posterior map that holds a share p of its mass, for up to CRED_MAX_LEVELS shares at once - a radix select on
// the float bits, most significant digit first, 8-bit digits, four passes.  Everything that is added is an integer (masses in 2^-44
// fixed point, counts), in LDS and at agent scope, so no number depends on the order of the additions or on who arrives last.
#include "kernels.h"
#include "tail_shared.h"

#include <algorithm>

namespace ccvpe {

typedef unsigned long long cred_u64;
static constexpr int CRED_SRC_MAP = 0, CRED_SRC_LOGITS = 1, CRED_SRC_PRIOR = 2;
#ifndef CCVPE_CREDIBLE_ONE_WG
#define CCVPE_CREDIBLE_ONE_WG 0   // dev builds (tools/build_variant.sh): 1 = stored maps run as ONE 512-thread workgroup per query, all passes out of
#endif                            // LDS in one launch - the launch shape the chunked one is timed against (no probe, timing only)
static constexpr int CRED_CELLS = TAIL_HW * TAIL_HW / TAIL_CHUNKS / 256;   // 16 cells per thread and pass
static_assert(CRED_CELLS == 16 && CRED_DIGITS == 256 && CRED_PASSES * 8 == 32 && CRED_MAX_LEVELS <= 8, "four 8-bit digits; a wave scans two levels at most");

// key and mass of a cell (include/ccvpe.h): NaN, zero and negative values have neither; the scaling by 2^44 is exact, the conversion truncates
__device__ __forceinline__ unsigned cred_key(float h) { return h > 0.f ? __float_as_uint(h) : 0u; }
__device__ __forceinline__ cred_u64 cred_mass(float h) { return h > 0.f ? (cred_u64)(fminf(h, 1.f) * 17592186044416.f) : 0ull; }
// T(p) of a total Q > 0: ceil(p Q) in float64, raised to 1 and capped at Q (the conversion of Q rounds, so the product may exceed it)
__device__ __forceinline__ cred_u64 cred_threshold(float level, cred_u64 Q) {
    const double t = ceil((double)level * (double)Q);
    cred_u64 T = t >= 9223372036854775808.0 ? Q : (cred_u64)t;
    if (T < 1ull) T = 1ull;
    return T > Q ? Q : T;
}

// The 16 values of this thread in chunk `lo` of query b.  A 16-byte aligned stored map and the logits sources are read as four float4
// (value hv[4 u + e] is cell lo + (tid + 256 u) * 4 + e), any other stored map value by value (hv[u] is cell lo + tid + 256 u); the
// return value says which.  Logits sources: posterior_value with the query's (m, inv) - the bits pose_argmax_kernel stores - and the
// all-zero map for a query without a finite posterior.  Whole chunks: every address lies inside the map
template <int SRC>
__device__ __forceinline__ bool cred_load(const CredibleParams& p, int b, int lo, float m, float inv, float (&hv)[CRED_CELLS], int t = threadIdx.x) {
    constexpr int n = TAIL_HW * TAIL_HW;
    if constexpr (SRC == CRED_SRC_MAP) {
        const float* h = p.belief + (size_t)b * n;
        if ((reinterpret_cast<uintptr_t>(h) & 15) == 0) {
            const float4* h4 = reinterpret_cast<const float4*>(h + lo);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float4 v = h4[t + u * 256];
                hv[4 * u] = v.x; hv[4 * u + 1] = v.y; hv[4 * u + 2] = v.z; hv[4 * u + 3] = v.w;
            }
            return true;
        }
#pragma unroll
        for (int u = 0; u < CRED_CELLS; ++u) hv[u] = h[lo + t + u * 256];
        return false;
    } else {
        float4 v[4];
        load_chunk<SRC == CRED_SRC_PRIOR>(p.logits + (size_t)b * n, SRC == CRED_SRC_PRIOR ? p.prior + (size_t)b * p.prior_stride : nullptr, lo, v);
        const bool fin = isfinite(m) && isfinite(inv);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            hv[4 * u] = fin ? posterior_value(v[u].x, m, inv) : 0.f; hv[4 * u + 1] = fin ? posterior_value(v[u].y, m, inv) : 0.f;
            hv[4 * u + 2] = fin ? posterior_value(v[u].z, m, inv) : 0.f; hv[4 * u + 3] = fin ? posterior_value(v[u].w, m, inv) : 0.f;
        }
        return true;
    }
}

// the map's value at cell i in [0, n) - the probe's read, behind the caller's range check
template <int SRC>
__device__ __forceinline__ float cred_value_at(const CredibleParams& p, int b, int i, float m, float inv) {
    constexpr int n = TAIL_HW * TAIL_HW;
    if constexpr (SRC == CRED_SRC_MAP) return p.belief[(size_t)b * n + i];
    else {
        float x = p.logits[(size_t)b * n + i];
        if constexpr (SRC == CRED_SRC_PRIOR) x += p.prior[(size_t)b * p.prior_stride + i];
        return isfinite(m) && isfinite(inv) ? posterior_value(x, m, inv) : 0.f;
    }
}

// One cell into row `row` of the workgroup's histogram.  Most cells of a sharp map, and all of a uniform one, share a digit: a wave
// whose lanes agree (all matching, one digit) sums its masses with xor shuffles and one lane adds; 64 lanes adding to one LDS word
// would serialise.  Every index is masked to the digit range
__device__ __forceinline__ void cred_add(cred_u64* lm, unsigned* lc, int row, bool match, unsigned digit, cred_u64 q) {
    if (!__any(match)) return;
    const int bin = match ? (int)(digit & (CRED_DIGITS - 1)) : -1;
    const int at = row * CRED_DIGITS + (int)(digit & (CRED_DIGITS - 1));
    if (__all(bin == __builtin_amdgcn_readfirstlane(bin))) {   // (every lane matches: bin >= 0, and the wave is whole - 64 cells)
        cred_u64 t = q;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
        if ((threadIdx.x & 63) == 0) {
            if (t) atomicAdd(&lm[at], t);
            atomicAdd(&lc[at], 64u);
        }
    } else if (match) {
        if (q) atomicAdd(&lm[at], q);
        atomicAdd(&lc[at], 1u);
    }
}

// One wave, one level: the digits of histogram row (lm, lc) from the top, carrying (above, cab) - the mass and count of the keys above
// this row's prefix - to the digit at which the carried mass first reaches T.  Lane l holds digits 255 - 4 l .. 252 - 4 l; an
// inclusive scan over the lanes, a ballot, and the lane that holds the digit walks its four.  Out, in every lane: the digit, the mass
// and count above it, and its own mass and count.  A row whose carried total stays below T (it cannot: above + the row's total is
// G(prefix) >= T) ends at digit 0 - an index inside the row either way
__device__ __forceinline__ void cred_scan(const cred_u64* lm, const unsigned* lc, cred_u64 above, unsigned cab, cred_u64 T, unsigned& digit,
                                          cred_u64& nabove, unsigned& ncab, cred_u64& bmass, unsigned& bcnt) {
    const int lane = threadIdx.x & 63;
    const int d0 = CRED_DIGITS - 1 - 4 * lane;
    const cred_u64 m0 = lm[d0], m1 = lm[d0 - 1], m2 = lm[d0 - 2], m3 = lm[d0 - 3];
    const unsigned c0 = lc[d0], c1 = lc[d0 - 1], c2 = lc[d0 - 2], c3 = lc[d0 - 3];
    const cred_u64 sm = m0 + m1 + m2 + m3;
    const unsigned sc = c0 + c1 + c2 + c3;
    cred_u64 im = sm;
    unsigned ic = sc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const cred_u64 tm = __shfl_up(im, off);
        const unsigned tc = __shfl_up(ic, off);
        if (lane >= off) { im += tm; ic += tc; }
    }
    const cred_u64 hit = __ballot(above + im >= T);
    const int src = hit ? __ffsll((long long)hit) - 1 : 63;
    cred_u64 a = above + im - sm, mm = m0;
    unsigned ca = cab + ic - sc, cc = c0, ds = (unsigned)d0;
    if (a + m0 < T) {
        a += m0; ca += c0; ds -= 1u; mm = m1; cc = c1;
        if (a + m1 < T) {
            a += m1; ca += c1; ds -= 1u; mm = m2; cc = c2;
            if (a + m2 < T) { a += m2; ca += c2; ds -= 1u; mm = m3; cc = c3; }
        }
    }
    digit = __shfl(ds, src) & (CRED_DIGITS - 1);
    nabove = __shfl(a, src); ncab = __shfl(ca, src);
    bmass = __shfl(mm, src); bcnt = __shfl(cc, src);
}

// Pass `pass` of CRED_PASSES, grid (64 chunks, B), 256 threads: chunk c of query b is belief_summary_kernel's / pose_argmax_kernel's
// chunk c.  FIRST (pass 0): no level has a prefix yet, so ONE histogram row over the top digit serves all levels; its totals are Q and
// the count of positive cells, and the probe's two sums - one comparison per cell - ride along.  Later passes: a row per level over the
// cells whose higher digits equal the level's prefix; levels that share a prefix share the row of the first of them (group[]).
// The workgroup's rows go to the query's rows with agent-scope integer adds (non-empty buckets only), then the ticket; the last arriver
// swaps the query's rows for zero - the read and the reset in one operation at the memory side -, scans each level (wave w: levels w
// and w + 4) and writes the state the next launch reads, the last pass the level columns of `cred`.
// Cells with key 0 - the whole of a delta map but one - touch nothing.  A query with Q == 0 is dead after pass 0: nothing is added and
// nothing scanned for it.
template <int SRC, bool FIRST>
__global__ __launch_bounds__(256) void credible_pass_kernel(const CredibleParams p, int pass) {
    constexpr int ROWS = FIRST ? 1 : CRED_MAX_LEVELS;
    __shared__ cred_u64 lm[ROWS * CRED_DIGITS];
    __shared__ unsigned lc[ROWS * CRED_DIGITS];
    __shared__ float gm, gs;
    __shared__ unsigned flag;
    __shared__ unsigned s_prefix[CRED_MAX_LEVELS], s_group[CRED_MAX_LEVELS], s_cab[CRED_MAX_LEVELS], s_gcnt[CRED_MAX_LEVELS];
    __shared__ cred_u64 s_T[CRED_MAX_LEVELS], s_above[CRED_MAX_LEVELS], s_gmass[CRED_MAX_LEVELS];
    __shared__ cred_u64 s_pm[4];
    __shared__ unsigned s_pc[4];
    constexpr int n = TAIL_HW * TAIL_HW, per = n / TAIL_CHUNKS;
    const int b = blockIdx.y, c = blockIdx.x, lo = c * per, tid = threadIdx.x;
    const int L = min(max(p.n_levels, 1), CRED_MAX_LEVELS);
    const int shift = 24 - 8 * min(max(pass, 0), CRED_PASSES - 1);
    const int cols = 4 + 3 * L;
    CredState* st = p.state + b;
    if constexpr (SRC != CRED_SRC_MAP) softmax_stats(p.partial, b, TAIL_CHUNKS, gm, gs);
    for (int i = tid; i < ROWS * CRED_DIGITS; i += 256) { lm[i] = 0ull; lc[i] = 0u; }
    bool alive = true;
    if constexpr (!FIRST) {
        alive = st->alive != 0u;
        if (tid < CRED_MAX_LEVELS) {
            s_prefix[tid] = st->prefix[tid]; s_group[tid] = tid < L && alive ? st->group[tid] : 0xffffffffu;
            s_T[tid] = st->T[tid]; s_above[tid] = st->above[tid]; s_cab[tid] = st->cabove[tid];
        }
    }
    __syncthreads();
    float m = 0.f, inv = 0.f;
    if constexpr (SRC != CRED_SRC_MAP) { m = gm; inv = gs; }
    if (alive) {
        float hv[CRED_CELLS];
        (void)cred_load<SRC>(p, b, lo, m, inv, hv);
        if constexpr (FIRST) {
            // the probe: the index is checked before the load; a bad one reads nothing and adds nothing
            const int pi = p.probe ? p.probe[b] : -1;
            const bool pv = (unsigned)pi < (unsigned)n;
            const unsigned pk = pv ? cred_key(cred_value_at<SRC>(p, b, pi, m, inv)) : 0xffffffffu;
            cred_u64 pa = 0ull;
            unsigned pr = 0u;
#pragma unroll
            for (int u = 0; u < CRED_CELLS; ++u) {
                const unsigned k = cred_key(hv[u]);
                const cred_u64 q = cred_mass(hv[u]);
                cred_add(lm, lc, 0, k != 0u, k >> 24, q);
                if (k > pk) { pa += q; pr += 1u; }
            }
            if (pv) {   // (uniform over the workgroup)
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) { pa += __shfl_xor(pa, off); pr += __shfl_xor(pr, off); }
                if ((tid & 63) == 0) { s_pm[tid >> 6] = pa; s_pc[tid >> 6] = pr; }
            }
            __syncthreads();
            if (pv && tid == 0) {
                const cred_u64 a = s_pm[0] + s_pm[1] + s_pm[2] + s_pm[3];
                const cred_u64 r = (cred_u64)s_pc[0] + s_pc[1] + s_pc[2] + s_pc[3];
                if (a) (void)__hip_atomic_fetch_add(p.pacc + (size_t)b * 2, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (r) (void)__hip_atomic_fetch_add(p.pacc + (size_t)b * 2 + 1, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else {
            for (int j = 0; j < L; ++j) {
                if (s_group[j] != (unsigned)j) continue;   // (uniform: this level's cells are counted in an earlier level's row)
                const unsigned want = s_prefix[j] >> (shift + 8);
#pragma unroll
                for (int u = 0; u < CRED_CELLS; ++u) {
                    const unsigned k = cred_key(hv[u]);
                    cred_add(lm, lc, j, k != 0u && (k >> (shift + 8)) == want, k >> shift, cred_mass(hv[u]));
                }
            }
            __syncthreads();
        }
        cred_u64* gmass = p.hmass + (size_t)b * CRED_MAX_LEVELS * CRED_DIGITS;
        unsigned* gcnt = p.hcnt + (size_t)b * CRED_MAX_LEVELS * CRED_DIGITS;
        for (int i = tid; i < (FIRST ? 1 : L) * CRED_DIGITS; i += 256) {
            const unsigned cn = lc[i];
            const cred_u64 ms = lm[i];
            if (cn) (void)__hip_atomic_fetch_add(gcnt + i, cn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (ms) (void)__hip_atomic_fetch_add(gmass + i, ms, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (!ticket_arrive(p.tickets + b, 1u, (unsigned)TAIL_CHUNKS, &flag)) return;
    if (!alive) return;

    // ---- last arriver of query b ----
    cred_u64* gmass = p.hmass + (size_t)b * CRED_MAX_LEVELS * CRED_DIGITS;
    unsigned* gcnt = p.hcnt + (size_t)b * CRED_MAX_LEVELS * CRED_DIGITS;
    for (int i = tid; i < (FIRST ? 1 : L) * CRED_DIGITS; i += 256) {
        lm[i] = __hip_atomic_exchange(gmass + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        lc[i] = __hip_atomic_exchange(gcnt + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    float* row = p.cred + (size_t)b * cols;
    cred_u64 Q = 0ull;
    if constexpr (FIRST) {
        unsigned np = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) { Q += lm[4 * lane + e]; np += lc[4 * lane + e]; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { Q += __shfl_xor(Q, off); np += __shfl_xor(np, off); }   // (every wave: the same integers)
        if (tid == 0) {
            const int pi = p.probe ? p.probe[b] : -1;
            const bool pv = (unsigned)pi < (unsigned)n;
            const cred_u64 pa = __hip_atomic_exchange(p.pacc + (size_t)b * 2, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const cred_u64 pr = __hip_atomic_exchange(p.pacc + (size_t)b * 2 + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            row[0] = (float)((double)Q * 5.684341886080802e-14);   // 2^-44
            row[1] = (float)np;
            row[2] = pv && Q ? (float)((double)pa / (double)Q) : NAN;
            row[3] = pv ? (float)pr : NAN;
            st->alive = Q ? 1u : 0u;
        }
        if (Q == 0ull) {
            if (tid < L) { row[4 + 3 * tid] = NAN; row[5 + 3 * tid] = 0.f; row[6 + 3 * tid] = NAN; }
            return;
        }
    }
    for (int j = wave; j < L; j += 4) {
        const cred_u64 T = FIRST ? cred_threshold(p.level[j], Q) : s_T[j];
        const int r = FIRST ? 0 : (int)(s_group[j] & (CRED_MAX_LEVELS - 1));
        unsigned digit, ncab, bcnt;
        cred_u64 nabove, bmass;
        cred_scan(lm + r * CRED_DIGITS, lc + r * CRED_DIGITS, FIRST ? 0ull : s_above[j], FIRST ? 0u : s_cab[j], T, digit, nabove, ncab, bmass, bcnt);
        if (lane == 0) {
            s_T[j] = T; s_above[j] = nabove; s_cab[j] = ncab;
            s_gmass[j] = nabove + bmass; s_gcnt[j] = ncab + bcnt;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) s_prefix[j] = (FIRST ? 0u : s_prefix[j]) | (digit << shift);   // (behind every lane's read of s_group / s_prefix above)
    }
    __syncthreads();
    if (tid < L) {
        const int j = tid;
        unsigned g = (unsigned)j;
        for (int e = j - 1; e >= 0; --e) if (s_prefix[e] == s_prefix[j]) g = (unsigned)e;
        st->T[j] = s_T[j]; st->above[j] = s_above[j]; st->cabove[j] = s_cab[j]; st->prefix[j] = s_prefix[j]; st->group[j] = g;
        if (shift == 0) {   // the key is complete: k*, C(k*) and G(k*) / Q
            cred_u64 total = Q;
            if constexpr (!FIRST) total = st->Q;
            row[4 + 3 * j] = __uint_as_float(s_prefix[j]);
            row[5 + 3 * j] = (float)s_gcnt[j];
            row[6 + 3 * j] = (float)((double)s_gmass[j] / (double)total);
        }
    }
    if constexpr (FIRST) { if (tid == 0) st->Q = Q; }
}

// The level map: cell i holds the number of levels whose region contains it, the levels k_i >= k*_j; all zero for a dead query.
// Grid (64 chunks, B), the passes' loads; four cells of a float4 leave as one 32-bit store where the output row is 4-byte aligned
template <int SRC>
__global__ __launch_bounds__(256) void credible_map_kernel(const CredibleParams p) {
    __shared__ float gm, gs;
    __shared__ unsigned s_k[CRED_MAX_LEVELS];
    constexpr int n = TAIL_HW * TAIL_HW, per = n / TAIL_CHUNKS;
    const int b = blockIdx.y, lo = blockIdx.x * per, tid = threadIdx.x;
    const int L = min(max(p.n_levels, 1), CRED_MAX_LEVELS);
    const CredState* st = p.state + b;
    if constexpr (SRC != CRED_SRC_MAP) softmax_stats(p.partial, b, TAIL_CHUNKS, gm, gs);
    if (tid < CRED_MAX_LEVELS) s_k[tid] = tid < L && st->alive != 0u ? st->prefix[tid] : 0xffffffffu;   // (no key reaches 2^32 - 1)
    __syncthreads();
    float m = 0.f, inv = 0.f;
    if constexpr (SRC != CRED_SRC_MAP) { m = gm; inv = gs; }
    float hv[CRED_CELLS];
    const bool vec = cred_load<SRC>(p, b, lo, m, inv, hv);
    unsigned cnt[CRED_CELLS];
#pragma unroll
    for (int u = 0; u < CRED_CELLS; ++u) cnt[u] = 0u;
    for (int j = 0; j < L; ++j) {
        const unsigned ks = s_k[j];
#pragma unroll
        for (int u = 0; u < CRED_CELLS; ++u) cnt[u] += cred_key(hv[u]) >= ks ? 1u : 0u;
    }
    unsigned char* out = p.level_map + (size_t)b * n + lo;
    if (vec && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            reinterpret_cast<unsigned*>(out)[tid + u * 256] = cnt[4 * u] | (cnt[4 * u + 1] << 8) | (cnt[4 * u + 2] << 16) | (cnt[4 * u + 3] << 24);
    } else if (vec) {
#pragma unroll
        for (int u = 0; u < CRED_CELLS; ++u) out[(tid + (u >> 2) * 256) * 4 + (u & 3)] = (unsigned char)cnt[u];
    } else {
#pragma unroll
        for (int u = 0; u < CRED_CELLS; ++u) out[tid + u * 256] = (unsigned char)cnt[u];
    }
}

#if CCVPE_CREDIBLE_ONE_WG
// The other launch shape, for timing: one workgroup per query of 512 threads walks the 64 chunks (two at a time, 256 threads each; 1024 threads spill) once per pass,
// histograms, scans and states in LDS, barriers between the passes, the level map as a fifth walk.  The probe columns are not computed.
__global__ __launch_bounds__(512) void credible_one_kernel(const CredibleParams p) {
    __shared__ cred_u64 lm[CRED_MAX_LEVELS * CRED_DIGITS];
    __shared__ unsigned lc[CRED_MAX_LEVELS * CRED_DIGITS];
    __shared__ unsigned s_prefix[CRED_MAX_LEVELS], s_group[CRED_MAX_LEVELS], s_cab[CRED_MAX_LEVELS], s_gcnt[CRED_MAX_LEVELS];
    __shared__ cred_u64 s_T[CRED_MAX_LEVELS], s_above[CRED_MAX_LEVELS], s_gmass[CRED_MAX_LEVELS], s_Q;
    constexpr int n = TAIL_HW * TAIL_HW, per = n / TAIL_CHUNKS;
    const int b = blockIdx.x, tid = threadIdx.x, t = tid & 255, grp = tid >> 8, lane = tid & 63, wave = tid >> 6;
    const int L = min(max(p.n_levels, 1), CRED_MAX_LEVELS);
    float* row = p.cred + (size_t)b * (4 + 3 * L);
    for (int pass = 0; pass < CRED_PASSES; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int i = tid; i < CRED_MAX_LEVELS * CRED_DIGITS; i += 512) { lm[i] = 0ull; lc[i] = 0u; }
        __syncthreads();
        for (int c = grp; c < TAIL_CHUNKS; c += 2) {
            float hv[CRED_CELLS];
            (void)cred_load<CRED_SRC_MAP>(p, b, c * per, 0.f, 0.f, hv, t);
            for (int j = 0; j < (pass == 0 ? 1 : L); ++j) {
                if (pass > 0 && s_group[j] != (unsigned)j) continue;
                const unsigned want = pass > 0 ? s_prefix[j] >> (shift + 8) : 0u;
#pragma unroll
                for (int u = 0; u < CRED_CELLS; ++u) {
                    const unsigned k = cred_key(hv[u]);
                    cred_add(lm, lc, j, k != 0u && (pass == 0 || (k >> (shift + 8)) == want), k >> shift, cred_mass(hv[u]));
                }
            }
        }
        __syncthreads();
        cred_u64 Q = 0ull;
        if (pass == 0) {
            unsigned np = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) { Q += lm[4 * lane + e]; np += lc[4 * lane + e]; }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { Q += __shfl_xor(Q, off); np += __shfl_xor(np, off); }
            if (tid == 0) { s_Q = Q; row[0] = (float)((double)Q * 5.684341886080802e-14); row[1] = (float)np; row[2] = NAN; row[3] = NAN; }
            if (Q == 0ull) {
                if (tid < L) { row[4 + 3 * tid] = NAN; row[5 + 3 * tid] = 0.f; row[6 + 3 * tid] = NAN; s_prefix[tid] = 0xffffffffu; }
                break;
            }
        }
        for (int j = wave; j < L; j += 8) {
            const int r = pass == 0 ? 0 : (int)(s_group[j] & (CRED_MAX_LEVELS - 1));
            unsigned digit, ncab, bcnt;
            cred_u64 nabove, bmass;
            const cred_u64 T = pass == 0 ? cred_threshold(p.level[j], Q) : s_T[j];
            cred_scan(lm + r * CRED_DIGITS, lc + r * CRED_DIGITS, pass == 0 ? 0ull : s_above[j], pass == 0 ? 0u : s_cab[j], T, digit, nabove, ncab, bmass, bcnt);
            if (lane == 0) {
                s_T[j] = T; s_above[j] = nabove; s_cab[j] = ncab; s_gmass[j] = nabove + bmass; s_gcnt[j] = ncab + bcnt;
                s_prefix[j] = (pass == 0 ? 0u : s_prefix[j]) | (digit << shift);
            }
        }
        __syncthreads();
        if (tid < L) {
            unsigned g = (unsigned)tid;
            for (int e = tid - 1; e >= 0; --e) if (s_prefix[e] == s_prefix[tid]) g = (unsigned)e;
            s_group[tid] = g;
            if (shift == 0) {
                row[4 + 3 * tid] = __uint_as_float(s_prefix[tid]); row[5 + 3 * tid] = (float)s_gcnt[tid];
                row[6 + 3 * tid] = (float)((double)s_gmass[tid] / (double)s_Q);
            }
        }
        __syncthreads();
    }
    if (!p.level_map) return;
    __syncthreads();
    for (int c = grp; c < TAIL_CHUNKS; c += 2) {
        float hv[CRED_CELLS];
        const bool vec = cred_load<CRED_SRC_MAP>(p, b, c * per, 0.f, 0.f, hv, t);
        unsigned char* out = p.level_map + (size_t)b * n + c * per;
#pragma unroll
        for (int u = 0; u < CRED_CELLS; ++u) {
            unsigned cnt = 0u;
            for (int j = 0; j < L; ++j) cnt += cred_key(hv[u]) >= s_prefix[j] ? 1u : 0u;
            out[vec ? (t + (u >> 2) * 256) * 4 + (u & 3) : t + u * 256] = (unsigned char)cnt;
        }
    }
}
#endif

template <int SRC>
static void credible_launches(const CredibleParams& p, hipStream_t s) {
    const dim3 grid(TAIL_CHUNKS, p.B), block(256);
    CCVPE_LAUNCH((credible_pass_kernel<SRC, true>), grid, block, 0, s, p, 0);
    for (int pass = 1; pass < CRED_PASSES; ++pass) CCVPE_LAUNCH((credible_pass_kernel<SRC, false>), grid, block, 0, s, p, pass);
    if (p.level_map) CCVPE_LAUNCH(credible_map_kernel<SRC>, grid, block, 0, s, p);
}

// [CRED_SLICE x 8 x 256 masses][CRED_SLICE x 2 probe sums][CRED_SLICE x 8 x 256 counts] - zero between launches, like the ticket counters -
// then [CRED_SLICE states]; a batch above CRED_SLICE queries runs in slices over the one region
size_t credible_zero_words(int B) {
    const size_t q = (size_t)std::min(B, CRED_SLICE);
    return q * (CRED_MAX_LEVELS * CRED_DIGITS * 3 + 4);
}
size_t credible_state_words(int B) { return (size_t)std::min(B, CRED_SLICE) * (sizeof(CredState) / sizeof(unsigned)); }

void credible_scratch(CredibleParams& p, int B, void* zeroed, void* state) {
    const size_t q = (size_t)std::min(B, CRED_SLICE);
    p.hmass = reinterpret_cast<cred_u64*>(zeroed);
    p.pacc = p.hmass + q * CRED_MAX_LEVELS * CRED_DIGITS;
    p.hcnt = reinterpret_cast<unsigned*>(p.pacc + q * 2);
    p.state = reinterpret_cast<CredState*>(state);
}

void launch_credible(const CredibleParams& p0, hipStream_t s) {
    constexpr size_t n = (size_t)TAIL_HW * TAIL_HW;
    const int cols = 4 + 3 * p0.n_levels;
    for (int b0 = 0; b0 < p0.B; b0 += CRED_SLICE) {
        CredibleParams p = p0;
        p.B = std::min(CRED_SLICE, p0.B - b0);
        if (p.belief) p.belief += b0 * n;
        if (p.logits) { p.logits += b0 * n; p.partial += (size_t)b0 * TAIL_CHUNKS * 2; }
        if (p.prior) p.prior += (long long)b0 * p.prior_stride;
        if (p.probe) p.probe += b0;
        p.cred += (size_t)b0 * cols;
        if (p.level_map) p.level_map += b0 * n;
#if CCVPE_CREDIBLE_ONE_WG
        if (p.belief) { CCVPE_LAUNCH(credible_one_kernel, dim3(p.B), dim3(512), 0, s, p); continue; }
#endif
        if (p.belief) credible_launches<CRED_SRC_MAP>(p, s);
        else if (p.prior) credible_launches<CRED_SRC_PRIOR>(p, s);
        else credible_launches<CRED_SRC_LOGITS>(p, s);
    }
}

}  // namespace ccvpe
