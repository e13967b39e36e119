// The decoder's transposed convolutions, ConvTranspose2d(k2, s2) (models.py:407-446), on a kernel of their own.
//
// As a GEMM the layer is [pixels x Cin] x [Cin x 4 cw] with a pixel-shuffle store: output pixel (2y + dy, 2x + dx) receives the
// column group (tap) q = 2 dy + dx of input pixel (y, x).  The general pointwise tiles (kernels_pw.hip) give a workgroup one column
// block, so the input is read and masked once per block (4-5 times per launch), and emit_out4 works the pixel-shuffle address out
// again for every 16-byte piece.  Here:
//   * a workgroup of eight waves stages the weights of ALL FOUR taps in LDS once (four-tap form), or - where they do not fit - the
//     two taps of one dy (two-tap form, grid y = 2): [taps * cw][K'] with K' the live channels only (below);
//   * a wave owns 16 consecutive input pixels per step and loads their channels straight into the MFMA operand registers, once,
//     unconditionally (rows past the end re-read the last row and are not stored), the next row tile in flight under the current
//     tile's MFMAs; the accumulators are channel-major (weights as the MFMA's first operand), cw / 16 * taps of them;
//   * the K loop walks a host-made list of 4-channel groups (deconv_k2s2_prepare): groups whose weights are all zero - the seven
//     unused channels behind the localisation decoder's score channel - are not loaded; a listed group's dead channels are masked
//     (select, not multiply: whatever the buffer holds there, NaN included, contributes nothing);
//   * (b, y, x) of a row is divided out once per row tile and lane; the row's output offset goes through LDS to the lanes that
//     store it, the taps are additions to it; a tap's 16 x cw result passes a wave-private LDS patch so that consecutive lanes
//     store consecutive 16-byte pieces of one output pixel's slice;
//   * persistent grid over XCD-contiguous runs of row tiles; no atomics, one summation order: the same bits on every launch.
#include "igemm_common.h"

#include <algorithm>

namespace ccvpe {

static constexpr int DK_WAVES = 8;                   // waves of a workgroup: two per SIMD with one workgroup per CU
static constexpr size_t DK_LDS_MAX = 160 * 1024;

// floats of LDS: weights [taps * cw][16 J + 4], bias [taps * cw], the waves' patches [16][cw + 4], row offsets [16] per wave, group table
static size_t deconv_k2s2_lds(int taps, int cw, int J) {
    return ((size_t)taps * cw * (16 * J + 4) + (size_t)taps * cw + (size_t)DK_WAVES * 16 * (cw + 4) + DK_WAVES * 16 + DeconvK2S2Params::MAX_GROUPS) * sizeof(float);
}

// (the narrow instantiations are held to 128 registers: two workgroups, four waves per SIMD, where the LDS holds two - these shapes wait
// for memory, not for the matrix pipe)
template <int JMAX, int CT, int TAPS>
__global__ __launch_bounds__(64 * DK_WAVES, (JMAX == 6 && CT <= 3 && CT * TAPS <= 8) ? 4 : 2) void deconv_k2s2_kernel(const DeconvK2S2Params p) {
    constexpr int CW = 16 * CT, NT = CT * TAPS, LDC = CW + 4, C4 = CW / 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int J = p.ngroups >> 2;          // 16-channel steps of the compacted K
    const int ldb = 16 * J + 4;            // (16 J + 4) / 4 odd: conflict-free 16-byte reads down the rows
    float* Bs = smem;                                          // [NT * 16][ldb]
    float* bias_s = Bs + NT * 16 * ldb;                        // [NT * 16]
    float* Cs = bias_s + NT * 16;                              // [waves][16][LDC]
    int* rowb = reinterpret_cast<int*>(Cs + DK_WAVES * 16 * LDC);   // [waves][16]
    int* gtab = rowb + DK_WAVES * 16;                          // [ngroups]: channel << 4 | mask

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = TAPS == 2 ? 2 * (int)blockIdx.y : 0;        // first tap of this workgroup
    const int M = p.B * p.H * p.W;

    // ---- group table, bias and the compacted, masked weights of this workgroup's taps -> LDS, once ----
    if (tid < p.ngroups) gtab[tid] = ((int)p.gch[tid] << 4) | (int)p.gmask[tid];
    if (tid < NT * 16) bias_s[tid] = p.bias[q0 * CW + tid];
    {
        const int g4 = p.ngroups;
        for (int i = tid; i < NT * 16 * g4; i += 64 * DK_WAVES) {
            const int n = i / g4, g = i - n * g4;
            const int c = p.gch[g], mk = p.gmask[g];
            f32x4 w = *reinterpret_cast<const f32x4*>(p.wpk + (size_t)(q0 * CW + n) * p.Kpad + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = (mk >> e) & 1 ? w[e] : 0.f;
            *reinterpret_cast<f32x4*>(Bs + n * ldb + g * 4) = w;
        }
    }
    __syncthreads();

    const int mtiles = (M + 15) >> 4;
    const int kq = lane >> 4, kq4 = 4 * kq;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    int mt = wg * DK_WAVES + wave;
    const int mt_stride = gridDim.x * DK_WAVES;
    if (mt >= mtiles) return;

    // this lane's 16-byte piece of every 16-channel step: channel offset and mask
    int gt[JMAX];
#pragma unroll
    for (int j = 0; j < JMAX; ++j) gt[j] = j < J ? gtab[j * 4 + kq] : 0;

    float* cw = Cs + wave * 16 * LDC;
    int* rb = rowb + wave * 16;
    const float* bp = Bs + (lane & 15) * ldb + kq4;

    f32x4 acur[JMAX], anext[JMAX];
    auto load_tile = [&](int mtile, f32x4* dst) {
        const int m = min(mtile * 16 + (lane & 15), M - 1);     // rows past the end: the last row again (never stored)
        const float* row = p.x + (size_t)m * p.in_ld;
#pragma unroll
        for (int j = 0; j < JMAX; ++j)
            if (j < J) dst[j] = *reinterpret_cast<const f32x4*>(row + (gt[j] >> 4));
    };
    load_tile(mt, acur);

    const int ow_ld = 2 * p.W * p.ld;                             // one output image row, floats
    f32x4 acc[NT];
    while (mt < mtiles) {
        load_tile(mt + mt_stride, anext);
        // output offset (floats, < 2^31) of tap (0, 0) of this lane's row; -1: a row past the end
        {
            const int m = mt * 16 + (lane & 15);
            const int t = fast_div(m, p.fdw_mul, p.fdw_shift);
            const int x = m - t * p.W;
            const int b = fast_div(t, p.fdh_mul, p.fdh_shift);
            const int y = t - b * p.H;
            const int o = ((b * 2 * p.H + 2 * y) * 2 * p.W + 2 * x) * p.ld + p.coff;
            if (lane < 16) rb[lane] = m < M ? o : -1;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < JMAX; ++j) {
            if (j < J) {
                f32x4 a = acur[j];
                if ((p.jmasked >> j) & 1) {     // uniform
#pragma unroll
                    for (int e = 0; e < 4; ++e) a[e] = (gt[j] >> e) & 1 ? a[e] : 0.f;
                }
                // two column tiles at a time, their MFMAs alternating: an fp32 MFMA's result is ready 40 cycles after issue, the next one
                // can issue after 32 - back to back on ONE accumulator every MFMA waits 8 cycles unless the SIMD's other wave fills them
                static_assert(NT % 2 == 0, "column tiles are taken in pairs");
#pragma unroll
                for (int t = 0; t < NT; t += 2) {
                    const f32x4 b0 = *reinterpret_cast<const f32x4*>(bp + t * 16 * ldb + j * 16);
                    const f32x4 b1 = *reinterpret_cast<const f32x4*>(bp + (t + 1) * 16 * ldb + j * 16);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(b0.x, a.x, acc[t], 0, 0, 0);
                    acc[t + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(b1.x, a.x, acc[t + 1], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(b0.y, a.y, acc[t], 0, 0, 0);
                    acc[t + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(b1.y, a.y, acc[t + 1], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(b0.z, a.z, acc[t], 0, 0, 0);
                    acc[t + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(b1.z, a.z, acc[t + 1], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(b0.w, a.w, acc[t], 0, 0, 0);
                    acc[t + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(b1.w, a.w, acc[t + 1], 0, 0, 0);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- per tap: + bias -> the wave's patch -> 16-byte pieces, consecutive lanes along one output pixel's slice ----
#pragma unroll
        for (int q = 0; q < TAPS; ++q) {
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                const f32x4 bv = *reinterpret_cast<const f32x4*>(bias_s + (q * CT + t) * 16 + kq4);
                *reinterpret_cast<f32x4*>(cw + (lane & 15) * LDC + t * 16 + kq4) = acc[q * CT + t] + bv;
            }
            __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0) only: this wave's LDS traffic is done; global loads / stores stay in flight
            __builtin_amdgcn_wave_barrier();
            const int toff = ((q0 + q) >> 1) * ow_ld + ((q0 + q) & 1) * p.ld;
#pragma unroll
            for (int r = 0; r < CT; ++r) {
                const int it = lane + 64 * r;       // 16 rows x C4 pieces = 64 CT items
                const int row = it / C4, c4 = it - row * C4;
                const int o = rb[row];
                const f32x4 v = *reinterpret_cast<const f32x4*>(cw + row * LDC + c4 * 4);
                if (o >= 0) *reinterpret_cast<f32x4*>(p.out + (size_t)(unsigned)(o + toff + c4 * 4)) = v;
                // two wait states behind every 16-byte store, as behind conv_wino4_kernel's (kernels_wino4.hip; tests/test_isa_hazard.py
                // checks the generated code)
                __builtin_amdgcn_sched_barrier(0);
                asm volatile("s_nop 1");
                __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_wave_barrier();
        }
#pragma unroll
        for (int j = 0; j < JMAX; ++j) acur[j] = anext[j];
        mt += mt_stride;
    }
}

static void make_fast_div(unsigned d, unsigned& mul, unsigned& shift) {   // as conv_igemm_prepare's
    unsigned l = 0;
    while ((1u << l) < d) ++l;
    mul = (unsigned)((((unsigned long long)1 << 32) * (((unsigned long long)1 << l) - d)) / d + 1);
    shift = l;
}

bool deconv_k2s2_prepare(DeconvK2S2Params& p, const unsigned char* live) {
    if (p.B <= 0 || p.H <= 0 || p.W <= 0 || p.Cin <= 0 || p.Cin % 4 || p.in_ld < p.Cin || p.in_ld % 4 || p.Kpad < p.Cin || p.Kpad % 4) return false;
    if (p.cw <= 0 || p.cw % 16 || p.cw > 80 || p.ld % 4 || p.coff % 4 || p.coff < 0 || p.coff + p.cw > p.ld) return false;
    // 32-bit element offsets in the kernel
    if ((double)p.B * p.H * p.W * p.in_ld >= 2147483647.0 || 4.0 * p.B * p.H * p.W * p.ld >= 2147483647.0) return false;
    int n = 0;
    unsigned jm = 0;
    for (int c = 0; c < p.Cin; c += 4) {
        int mk = 0;
        for (int e = 0; e < 4; ++e) mk |= (!live || live[c + e]) ? 1 << e : 0;
        if (!mk) continue;
        if (n == DeconvK2S2Params::MAX_GROUPS) return false;
        p.gch[n] = (unsigned short)c; p.gmask[n] = (unsigned char)mk;
        if (mk != 15) jm |= 1u << (n >> 2);
        ++n;
    }
    if (n == 0) { p.gch[0] = 0; p.gmask[0] = 0; jm |= 1u; n = 1; }   // (no live channel: the bias alone)
    while (n % 4) {   // masked groups up to a whole 16-channel step
        p.gch[n] = 0; p.gmask[n] = 0; jm |= 1u << (n >> 2); ++n;
    }
    p.ngroups = n; p.jmasked = jm;
    const int J = n / 4, ct = p.cw / 16;
    if (ct <= 4 && deconv_k2s2_lds(4, p.cw, J) <= DK_LDS_MAX) p.taps = 4;
    else if (ct >= 3 && deconv_k2s2_lds(2, p.cw, J) <= DK_LDS_MAX) p.taps = 2;
    else return false;
    make_fast_div((unsigned)p.W, p.fdw_mul, p.fdw_shift);
    make_fast_div((unsigned)p.H, p.fdh_mul, p.fdh_shift);
    return true;
}

template <int JMAX, int CT, int TAPS>
static void launch_dk(const DeconvK2S2Params& p, hipStream_t s) {
    const size_t lds = deconv_k2s2_lds(TAPS, p.cw, p.ngroups / 4);
    static LdsAttr attr;
    auto kern = deconv_k2s2_kernel<JMAX, CT, TAPS>;
    ensure_dynamic_lds(attr, reinterpret_cast<const void*>(kern), lds);
    const int mtiles = (p.B * p.H * p.W + 15) / 16;
    const int ny = 4 / TAPS;
    // workgroups (eight waves each) a CU holds at once, by LDS and registers: at most two - the grid is the resident workgroups
    // (asked of the runtime once per instantiation, LDS size and device)
    static size_t occ_lds[16] = {0};
    static int occ[16] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = 0;
    if (occ_lds[dev] != lds) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, 64 * DK_WAVES, lds) != hipSuccess) { (void)hipGetLastError(); n = 1; }
        occ[dev] = std::max(1, std::min(2, n)); occ_lds[dev] = lds;
    }
    const int per_cu = occ[dev];
    const int gx = std::max(1, std::min((mtiles + DK_WAVES - 1) / DK_WAVES, 256 * per_cu / ny));
    CCVPE_LAUNCH(kern, dim3(gx, ny), dim3(64 * DK_WAVES), lds, s, p);
}

template <int JMAX>
static void launch_dk_j(const DeconvK2S2Params& p, hipStream_t s) {
    const int ct = p.cw / 16;
    if (p.taps == 4) {
        if (ct == 1) launch_dk<JMAX, 1, 4>(p, s);
        else if (ct == 2) launch_dk<JMAX, 2, 4>(p, s);
        else if (ct == 3) launch_dk<JMAX, 3, 4>(p, s);
        else launch_dk<JMAX, 4, 4>(p, s);
    } else {
        if (ct == 3) launch_dk<JMAX, 3, 2>(p, s);
        else if (ct == 4) launch_dk<JMAX, 4, 2>(p, s);
        else launch_dk<JMAX, 5, 2>(p, s);
    }
}

// p: as deconv_k2s2_prepare left it (it returned true)
void launch_deconv_k2s2(const DeconvK2S2Params& p, hipStream_t s) {
    if (p.ngroups <= 24) launch_dk_j<6>(p, s);
    else launch_dk_j<12>(p, s);
}

}  // namespace ccvpe
