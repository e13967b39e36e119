// Decoder level 6 with the transposed conv composed into the first 3x3 conv (reference models.py:42-47, 516-518, 633-635).
//
//   x[B,8,8,K] -> deconv6 (k2 s2, K -> 1024) -> cat [1024 | sat_block15 320] -> conv6.0 3x3 (1344 -> N) -> ReLU
//
// has no non-linearity between the transposed conv and conv6.0, so the 1024-channel half of conv6.0 is, per output parity class
// (py, px), a 2x2-tap convolution K -> N on the 8x8 input grid (the index algebra of compose_level1, ccvpe_weights.hip).  Each class
// runs as Winograd F(MxM,2x2) on 8/M x 8/M tiles: (M+1)^2 positions per class, one K x N weight matrix per (class, position).
//
//   level6_transform   x -> V[group = class*P + position][row = tile of sample][Kc]      (B^T d B, zeros outside the grid)
//   level6_gemm        M'[g] = V[g] . Wc[g]^T for the 4 P groups, fp32 MFMA (v_mfma_f32_32x32x2_f32, exact fp32)
//   (the skip half of conv6.0, 320 channels of sat_block15, is an ordinary 3x3 convolution launch without bias)
//   level6_combine     A^T M' A per (class, tile, channel) + skip half + border-case bias + ReLU -> conv6.0's output tensor
//
// M and the transform matrices are compile-time parameters (Wino<M>): F(4x4,2x2), 25 positions, 1.5625 K N products per output pixel of
// a class; F(2x2,2x2), 9 positions, 2.25 K N, four times the rows per group and 0.36 of the weight bytes.
// The weights come from level6_compose (fp64, once per handle): see ensure_level6 (ccvpe_weights.hip).
// The level's two remaining 3x3 layers, conv6.2 and conv6.0's skip half, run on the same GEMM in split form F(4x4,3x3): split6_transform,
// level6_gemm over 36 groups, split6_inverse (Split6Params, below the combine kernel).
#include "igemm_common.h"

namespace ccvpe {

// Cook-Toom matrices of the correlation y[i] = sum_k d[i + k] g[k], i < M, k < 2: y = A^T [(G g) * (B^T d)].
// F(4,2): points 0, 1, -1, 2, inf; F(2,2): points 0, 1, inf.  tests/level6_ref.py restates them; tests/test_level6_compose_cpu.py checks them.
template <int M> struct Wino;
template <> struct Wino<4> {
    static constexpr int NP = 5;
    static __host__ __device__ constexpr float bt(int u, int i) {
        constexpr float t[5][5] = {{2, -1, -2, 1, 0}, {0, -2, -1, 1, 0}, {0, 2, -3, 1, 0}, {0, -1, 0, 1, 0}, {0, 2, -1, -2, 1}};
        return t[u][i];
    }
    static __host__ __device__ constexpr float at(int i, int u) {
        constexpr float t[4][5] = {{1, 1, 1, 1, 0}, {0, 1, -1, 2, 0}, {0, 1, 1, 4, 0}, {0, 1, -1, 8, 1}};
        return t[i][u];
    }
    static __host__ __device__ constexpr double g(int u, int a) {
        constexpr double t[5][2] = {{0.5, 0.0}, {-0.5, -0.5}, {-1.0 / 6.0, 1.0 / 6.0}, {1.0 / 6.0, 1.0 / 3.0}, {0.0, 1.0}};
        return t[u][a];
    }
};
template <> struct Wino<2> {
    static constexpr int NP = 3;
    static __host__ __device__ constexpr float bt(int u, int i) {
        constexpr float t[3][3] = {{-1, 1, 0}, {0, 1, 0}, {0, -1, 1}};
        return t[u][i];
    }
    static __host__ __device__ constexpr float at(int i, int u) {
        constexpr float t[2][3] = {{1, 1, 0}, {0, 1, 1}};
        return t[i][u];
    }
    static __host__ __device__ constexpr double g(int u, int a) {
        constexpr double t[3][2] = {{-1.0, 0.0}, {1.0, 1.0}, {0.0, 1.0}};
        return t[u][a];
    }
};

int level6_positions(int wm) { return (wm + 1) * (wm + 1); }
// rows of one group (tiles of all samples, padded with zero rows to the GEMM's tile height) and that tile height
int level6_rows(int B, int wm, int* bm_out) {
    const int t = 8 / wm, rows = B * t * t;
    const int bm = rows > 64 ? 128 : rows > 32 ? 64 : 32;
    if (bm_out) *bm_out = bm;
    return (rows + bm - 1) / bm * bm;
}

// ---- input transform --------------------------------------------------------------------------------------------------------------
// grid (ceil(Kc / 4 / 128), R, 4 classes): one thread = 4 channels of one (class, tile).  The window of class (py, px), tile (ty, tx)
// starts at input pixel (M ty - 1 + py, M tx - 1 + px); pixels outside the 8x8 grid are zeros (they hold exactly the transposed-conv
// pixels outside the 16x16 map, so zero input reproduces conv6.0's zero padding).  Rows past the last tile and channels K .. Kc are zeros.
template <int M>
__global__ __launch_bounds__(128) void level6_transform_kernel(const Level6Params p) {
    using W = Wino<M>;
    constexpr int NP = W::NP, T = 8 / M;
    const int k = (blockIdx.x * 128 + threadIdx.x) * 4;
    if (k >= p.Kc) return;
    const int row = blockIdx.y, cls = blockIdx.z;
    const int b = row / (T * T), t = row - b * (T * T);
    const int y0 = M * (t / T) - 1 + (cls >> 1), x0 = M * (t % T) - 1 + (cls & 1);
    const bool live = b < p.B && k < p.K;
    f32x4 d[NP][NP];
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int y = y0 + i, x = x0 + j;
            d[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (live && (unsigned)y < 8u && (unsigned)x < 8u) d[i][j] = *reinterpret_cast<const f32x4*>(p.x + ((size_t)(b * 8 + y) * 8 + x) * p.K + k);
        }
    f32x4 c[NP][NP];   // B^T d
#pragma unroll
    for (int u = 0; u < NP; ++u)
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < NP; ++i)
                if (W::bt(u, i) != 0.f) s += W::bt(u, i) * d[i][j];
            c[u][j] = s;
        }
    float* dst = p.v + ((size_t)cls * NP * NP * p.R + row) * p.Kc + k;
    const size_t gstride = (size_t)p.R * p.Kc;
#pragma unroll
    for (int u = 0; u < NP; ++u)
#pragma unroll
        for (int v = 0; v < NP; ++v) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NP; ++j)
                if (W::bt(v, j) != 0.f) s += W::bt(v, j) * c[u][j];
            *reinterpret_cast<f32x4*>(dst + (size_t)(u * NP + v) * gstride) = s;
            // the next position's arithmetic reuses this store's registers at once: two wait states behind every 16-byte store, as
            // behind conv_wino4_kernel's (kernels_wino4.hip; tests/test_isa_hazard.py checks the generated code)
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_nop 1");
            __builtin_amdgcn_sched_barrier(0);
        }
}

// ---- grouped GEMM -----------------------------------------------------------------------------------------------------------------
// M'[g][r][n] = sum_k V[g][r][k] Wc[g][n][k]: the K loop of conv_igemm_kernel (kernels_igemm.hip: 32-deep tiles, register-staged into a
// double-buffered LDS image with 144-byte rows, one barrier per tile, weights as the MFMA's first operand so that accumulators are
// channel-major) without the gather: both operands are dense K-contiguous rows, padded (R to BM, Npad to 128, Kc to 32) so that no
// load needs a bound.  One workgroup = BM x 128 outputs of one group.  A group's weight panel is read by R / BM row blocks only (one at
// batch 32): the weights stream from HBM once per launch, the n-blocks of a group share its V rows through the L2 of one XCD (xcd_remap).
template <int BM, int WGM, int WGN>
__global__ __launch_bounds__(256) void level6_gemm_kernel(const Level6Params p) {
    constexpr int BN = 128, MT = 32;
    constexpr int WM = BM / WGM, WN = BN / WGN, TM = WM / MT, TN = WN / MT;
    static_assert(WGM * WGN == 4 && TM >= 1 && TN >= 1 && TM * MT * WGM == BM && TN * MT * WGN == BN, "whole MFMA tiles, 4 waves");
    constexpr int AR = BM / 32, BR = BN / 32;
    constexpr int KSTEP = 8, NKK = BK / KSTEP;

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                 // [2][BM][LDK]
    float* Bs = smem + 2 * BM * LDK;  // [2][BN][LDK]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int nbn = p.Npad / BN, mblocks = p.R / BM;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int nb = lid % nbn, rest = lid / nbn;
    const int mb = rest % mblocks, g = rest / mblocks;
    const int m0 = mb * BM, n0 = nb * BN;
    const int kq = tid & 7, r0 = tid >> 3;

    const float* arow = p.v + ((size_t)g * p.R + m0 + r0) * p.Kc + kq * 4;
    const float* brow = p.wc + ((size_t)g * p.Npad + n0 + r0) * p.Kc + kq * 4;
    const size_t rstep = (size_t)32 * p.Kc;

    f32x4 ra[AR], rb[BR];
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nkt = p.Kc / BK;
#pragma unroll
    for (int j = 0; j < AR; ++j) ra[j] = *reinterpret_cast<const f32x4*>(arow + j * rstep);
#pragma unroll
    for (int j = 0; j < BR; ++j) rb[j] = *reinterpret_cast<const f32x4*>(brow + j * rstep);
#pragma unroll
    for (int j = 0; j < AR; ++j) *reinterpret_cast<f32x4*>(As + (r0 + 32 * j) * LDK + kq * 4) = ra[j];
#pragma unroll
    for (int j = 0; j < BR; ++j) *reinterpret_cast<f32x4*>(Bs + (r0 + 32 * j) * LDK + kq * 4) = rb[j];
    __syncthreads();

    const int a_row = wm * WM + (lane & 31);
    const int b_row = wn * WN + (lane & 31);
    const int k_lane = (lane >> 5) * 4;

    for (int kt = 0; kt < nkt; ++kt) {
        const int stage = kt & 1;
        const int ktn = min(kt + 1, nkt - 1);   // unconditional prefetch (the last iteration re-reads its own tile: 1 of ~41)
#pragma unroll
        for (int j = 0; j < AR; ++j) ra[j] = *reinterpret_cast<const f32x4*>(arow + j * rstep + ktn * BK);
#pragma unroll
        for (int j = 0; j < BR; ++j) rb[j] = *reinterpret_cast<const f32x4*>(brow + j * rstep + ktn * BK);
        __builtin_amdgcn_sched_barrier(0);   // the prefetch stays above the MFMA block (kernels_igemm.hip)
        const float* as = As + stage * BM * LDK + a_row * LDK + k_lane;
        const float* bs = Bs + stage * BN * LDK + b_row * LDK + k_lane;
        f32x4 a[2][TM], b[2][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) a[0][i] = *reinterpret_cast<const f32x4*>(as + i * MT * LDK);
#pragma unroll
        for (int j = 0; j < TN; ++j) b[0][j] = *reinterpret_cast<const f32x4*>(bs + j * MT * LDK);
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
            const int cur = kk & 1, nxt = cur ^ 1;
            if (kk + 1 < NKK) {
#pragma unroll
                for (int i = 0; i < TM; ++i) a[nxt][i] = *reinterpret_cast<const f32x4*>(as + i * MT * LDK + (kk + 1) * KSTEP);
#pragma unroll
                for (int j = 0; j < TN; ++j) b[nxt][j] = *reinterpret_cast<const f32x4*>(bs + j * MT * LDK + (kk + 1) * KSTEP);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[cur][j].x, a[cur][i].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[cur][j].y, a[cur][i].y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[cur][j].z, a[cur][i].z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[cur][j].w, a[cur][i].w, acc[i][j], 0, 0, 0);
                }
        }
        __builtin_amdgcn_sched_barrier(0);   // ... and the LDS stores below it
#pragma unroll
        for (int j = 0; j < AR; ++j) *reinterpret_cast<f32x4*>(As + (stage ^ 1) * BM * LDK + (r0 + 32 * j) * LDK + kq * 4) = ra[j];
#pragma unroll
        for (int j = 0; j < BR; ++j) *reinterpret_cast<f32x4*>(Bs + (stage ^ 1) * BN * LDK + (r0 + 32 * j) * LDK + kq * 4) = rb[j];
        __syncthreads();
    }

    // epilogue: accumulators -> LDS C tile [BM][BN + 4] (the staging buffers are dead), rows leave as 16-byte stores
    constexpr int LDC = BN + 4;
    float* Cs = smem;
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int nl = wn * WN + j * MT + 8 * q + 4 * (lane >> 5);   // lane holds column m = lane & 31, rows n = 8 q + 4 (lane >> 5) + 0..3
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int ml = wm * WM + i * MT + (lane & 31);
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * q + e];
                *reinterpret_cast<f32x4*>(Cs + ml * LDC + nl) = v;
            }
        }
    __syncthreads();
    constexpr int C4 = BN / 4;
    for (int it = tid; it < BM * C4; it += 256) {
        const int ml = it / C4, c4 = it - ml * C4;
        const int n = n0 + c4 * 4;
        if (n >= p.N) continue;
        *reinterpret_cast<f32x4*>(p.mp + ((size_t)g * p.R + m0 + ml) * p.N + n) = *reinterpret_cast<const f32x4*>(Cs + ml * LDC + c4 * 4);
    }
}

// ---- combine ----------------------------------------------------------------------------------------------------------------------
// grid (ceil(N / 4 / 64), tiles of all samples, 4 classes): one thread = 4 channels of one (class, tile): Y = A^T M' A, then per output
// pixel (2 (M ty + i) + py, 2 (M tx + j) + px): (Y + skip half) + bc[border case], ReLU, one 16-byte store.  The same order for every
// pixel, no atomics: the same bits in every run.
template <int M>
__global__ __launch_bounds__(64) void level6_combine_kernel(const Level6Params p) {
    using W = Wino<M>;
    constexpr int NP = W::NP, T = 8 / M;
    const int n = (blockIdx.x * 64 + threadIdx.x) * 4;
    if (n >= p.N) return;
    const int row = blockIdx.y, cls = blockIdx.z;
    const int b = row / (T * T), t = row - b * (T * T);
    const int ty = t / T, tx = t - ty * T, py = cls >> 1, px = cls & 1;
    const float* src = p.mp + ((size_t)cls * NP * NP * p.R + row) * p.N + n;
    const size_t gstride = (size_t)p.R * p.N;
    f32x4 m[NP][NP];
#pragma unroll
    for (int u = 0; u < NP; ++u)
#pragma unroll
        for (int v = 0; v < NP; ++v) m[u][v] = *reinterpret_cast<const f32x4*>(src + (size_t)(u * NP + v) * gstride);
    f32x4 c[M][NP];   // A^T M'
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int v = 0; v < NP; ++v) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int u = 0; u < NP; ++u)
                if (W::at(i, u) != 0.f) s += W::at(i, u) * m[u][v];
            c[i][v] = s;
        }
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < M; ++j) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int v = 0; v < NP; ++v)
                if (W::at(j, v) != 0.f) s += W::at(j, v) * c[i][v];
            const int oy = 2 * (M * ty + i) + py, ox = 2 * (M * tx + j) + px;
            const int rcase = oy == 0 ? 1 : oy == 15 ? 2 : 0, ccase = ox == 0 ? 1 : ox == 15 ? 2 : 0;
            const size_t e = ((size_t)(b * 16 + oy) * 16 + ox) * p.N + n;
            s += *reinterpret_cast<const f32x4*>(p.skip + e);
            s += *reinterpret_cast<const f32x4*>(p.bc + (rcase * 3 + ccase) * p.N + n);
#pragma unroll
            for (int q = 0; q < 4; ++q) s[q] = fmaxf(s[q], 0.f);
            *reinterpret_cast<f32x4*>(p.out + e) = s;
        }
}

// ---- a 3x3 layer on the 16 x 16 map in split form (Split6Params) ---------------------------------------------------------------------
// F(4x4,3x3), points 0, +-1, +-2, inf: the B^T and A^T of kernels_wino4.hip (w4_bt, w4_at), so conv_wino4_filter's G g G^T are its
// weights.  tests/split_wino_ref.py restates the three matrices; tests/test_level6_split_cpu.py checks them.
struct Wino43 {
    static __host__ __device__ constexpr float bt(int u, int i) {
        constexpr float t[6][6] = {{4, 0, -5, 0, 1, 0}, {0, -4, -4, 1, 1, 0}, {0, 4, -4, -1, 1, 0}, {0, -2, -1, 2, 1, 0}, {0, 2, -1, -2, 1, 0}, {0, 4, 0, -5, 0, 1}};
        return t[u][i];
    }
    static __host__ __device__ constexpr float at(int i, int u) {
        constexpr float t[4][6] = {{1, 1, 1, 1, 1, 0}, {0, 1, -1, 2, -2, 0}, {0, 1, 1, 4, 4, 0}, {0, 1, -1, 8, -8, 1}};
        return t[i][u];
    }
};

// The tile height of the 36-group launches: at least eight row blocks per position where the rows allow it.  With 128-row tiles batch 32
// is 720 workgroups, 2.8 per CU at two resident: 87 TFLOP/s against 104 - 108 with 64-row tiles (1440); at batch 8 and 16 the 32-row
// tiles measured fastest (profiles/level6_split_trace_b32_fp32.md).  The composed launch keeps level6_rows.
int split6_rows(int B, int* bm_out) {
    const int rows = 16 * B;
    const int bm = rows >= 1024 ? 128 : rows >= 512 ? 64 : 32;
    if (bm_out) *bm_out = bm;
    return (rows + bm - 1) / bm * bm;
}

// One thread = 4 channels of one tile (row = 16 b + 4 ty + tx; threads run over (row, channel quad), quads fastest).  The tile's 6 x 6
// window starts at pixel (4 ty - 1, 4 tx - 1); pixels outside the map are zeros (pad 1).  Rows past the last tile and channels C .. Kc
// are written as zeros: the GEMM reads them unguarded.
__global__ __launch_bounds__(128) void split6_transform_kernel(const Split6Params p) {
    using W = Wino43;
    const int k4n = p.Kc >> 2;
    const int idx = blockIdx.x * 128 + threadIdx.x;
    if (idx >= p.R * k4n) return;
    const int row = idx / k4n, k = (idx - row * k4n) * 4;
    const int b = row >> 4, t = row & 15;
    const int y0 = 4 * (t >> 2) - 1, x0 = 4 * (t & 3) - 1;
    const bool live = b < p.B && k < p.C;
    f32x4 d[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int y = y0 + i, x = x0 + j;
            d[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (live && (unsigned)y < 16u && (unsigned)x < 16u)
                d[i][j] = *reinterpret_cast<const f32x4*>(p.x + ((size_t)(b * 16 + y) * 16 + x) * p.x_ld + p.x_coff + k);
        }
    f32x4 c[6][6];   // B^T d
#pragma unroll
    for (int u = 0; u < 6; ++u)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 6; ++i)
                if (W::bt(u, i) != 0.f) s += W::bt(u, i) * d[i][j];
            c[u][j] = s;
        }
    float* dst = p.v + (size_t)row * p.Kc + k;
    const size_t gstride = (size_t)p.R * p.Kc;
#pragma unroll
    for (int u = 0; u < 6; ++u)
#pragma unroll
        for (int v = 0; v < 6; ++v) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 6; ++j)
                if (W::bt(v, j) != 0.f) s += W::bt(v, j) * c[u][j];
            *reinterpret_cast<f32x4*>(dst + (size_t)(u * 6 + v) * gstride) = s;
            // two wait states behind every 16-byte store, as in level6_transform_kernel
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_nop 1");
            __builtin_amdgcn_sched_barrier(0);
        }
}

// One thread = 4 output channels of one tile: Y = A^T M' A, then per output pixel (4 ty + i, 4 tx + j): + bias, ReLU, one 16-byte store.
// The same order for every pixel, no atomics: the same bits in every run.
__global__ __launch_bounds__(64) void split6_inverse_kernel(const Split6Params p) {
    using W = Wino43;
    const int n4n = p.N >> 2;
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= 16 * p.B * n4n) return;
    const int row = idx / n4n, n = (idx - row * n4n) * 4;
    const int b = row >> 4, t = row & 15, ty = t >> 2, tx = t & 3;
    const float* src = p.mp + (size_t)row * p.N + n;
    const size_t gstride = (size_t)p.R * p.N;
    f32x4 m[6][6];
#pragma unroll
    for (int u = 0; u < 6; ++u)
#pragma unroll
        for (int v = 0; v < 6; ++v) m[u][v] = *reinterpret_cast<const f32x4*>(src + (size_t)(u * 6 + v) * gstride);
    f32x4 c[4][6];   // A^T M'
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int v = 0; v < 6; ++v) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int u = 0; u < 6; ++u)
                if (W::at(i, u) != 0.f) s += W::at(i, u) * m[u][v];
            c[i][v] = s;
        }
    f32x4 bias = {0.f, 0.f, 0.f, 0.f};
    if (p.bias) bias = *reinterpret_cast<const f32x4*>(p.bias + n);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int v = 0; v < 6; ++v)
                if (W::at(j, v) != 0.f) s += W::at(j, v) * c[i][v];
            s += bias;
            if (p.relu) {
#pragma unroll
                for (int q = 0; q < 4; ++q) s[q] = fmaxf(s[q], 0.f);
            }
            *reinterpret_cast<f32x4*>(p.out + ((size_t)(b * 16 + 4 * ty + i) * 16 + 4 * tx + j) * p.out_ld + p.out_coff + n) = s;
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_nop 1");
            __builtin_amdgcn_sched_barrier(0);
        }
}

bool split6_supported(const Split6Params& p) {
    int bm = 0;
    return p.B > 0 && p.B <= (1 << 20) && p.C > 0 && p.C % 4 == 0 && p.Kc % BK == 0 && p.Kc >= p.C && p.N > 0 && p.N % 4 == 0 && p.Npad % 128 == 0 &&
           p.Npad >= p.N && p.R == split6_rows(p.B, &bm) && p.bm == bm && p.x_ld % 4 == 0 && p.x_coff % 4 == 0 && p.x_coff + p.C <= p.x_ld &&
           p.out_ld % 4 == 0 && p.out_coff % 4 == 0 && p.out_coff + p.N <= p.out_ld && (long long)p.R * (p.Kc / 4) < (1ll << 31) &&
           (long long)36 * (p.R / p.bm) * (p.Npad / 128) < (1ll << 31);
}

Level6Params split6_gemm_params(const Split6Params& p) {
    Level6Params q{};
    q.wm = 4; q.B = p.B; q.K = p.C; q.Kc = p.Kc; q.N = p.N; q.Npad = p.Npad; q.R = p.R; q.bm = p.bm; q.groups = 36;
    q.v = p.v; q.wc = p.wc; q.mp = p.mp;
    return q;
}

void launch_split6_transform(const Split6Params& p, hipStream_t s) {
    CCVPE_LAUNCH(split6_transform_kernel, dim3((unsigned)((p.R * (p.Kc / 4) + 127) / 128)), dim3(128), 0, s, p);
}

void launch_split6_inverse(const Split6Params& p, hipStream_t s) {
    CCVPE_LAUNCH(split6_inverse_kernel, dim3((unsigned)((16 * p.B * (p.N / 4) + 63) / 64)), dim3(64), 0, s, p);
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
bool level6_supported(const Level6Params& p) {
    int bm = 0;
    return (p.wm == 4 || p.wm == 2) && p.groups == 4 * level6_positions(p.wm) && p.B > 0 && p.K > 0 && p.K % 4 == 0 && p.Kc % BK == 0 && p.Kc >= p.K && p.N > 0 && p.N % 4 == 0 &&
           p.Npad % 128 == 0 && p.Npad >= p.N && p.R == level6_rows(p.B, p.wm, &bm) && p.bm == bm;
}

void launch_level6_transform(const Level6Params& p, hipStream_t s) {
    const dim3 grid((p.Kc / 4 + 127) / 128, p.R, 4);
    if (p.wm == 4) CCVPE_LAUNCH(level6_transform_kernel<4>, grid, dim3(128), 0, s, p);
    else CCVPE_LAUNCH(level6_transform_kernel<2>, grid, dim3(128), 0, s, p);
}

template <int BM, int WGM, int WGN>
static void launch_gemm_t(const Level6Params& p, hipStream_t s) {
    constexpr size_t lds = std::max<size_t>(2 * (BM + 128) * LDK, BM * (128 + 4)) * sizeof(float);
    static LdsAttr attr;
    auto kern = level6_gemm_kernel<BM, WGM, WGN>;
    ensure_dynamic_lds(attr, reinterpret_cast<const void*>(kern), lds);
    const int blocks = p.groups * (p.R / BM) * (p.Npad / 128);
    CCVPE_LAUNCH(kern, dim3(blocks), dim3(256), lds, s, p);
}
void launch_level6_gemm(const Level6Params& p, hipStream_t s) {
    if (p.bm == 128) launch_gemm_t<128, 2, 2>(p, s);
    else if (p.bm == 64) launch_gemm_t<64, 2, 2>(p, s);
    else launch_gemm_t<32, 1, 4>(p, s);
}

void launch_level6_combine(const Level6Params& p, hipStream_t s) {
    const int t = 8 / p.wm;
    const dim3 grid((p.N / 4 + 63) / 64, p.B * t * t, 4);
    if (p.wm == 4) CCVPE_LAUNCH(level6_combine_kernel<4>, grid, dim3(64), 0, s, p);
    else CCVPE_LAUNCH(level6_combine_kernel<2>, grid, dim3(64), 0, s, p);
}

// ---- weight composition (once per handle) -------------------------------------------------------------------------------------------
// conv6.0 pixel (2I + py, 2J + px), tap (ky, kx) reads transposed-conv pixel (2I + py + ky - 1, ...) = input pixel (I - 1 + py + a,
// J - 1 + px + b) at parity (ty & 1, tx & 1), ty = py + ky + 1, a = (ty >> 1) - py (likewise for x), so
//   W2[py][px][a][b][n][k] = sum over the taps landing in window (a, b) of sum_m Wa[n][m][ky][kx] Wd[k][m][ty & 1][tx & 1]
// in double, from the PACKED fp32 weights of the two layers (so the derivation also runs behind ccvpe_load_packed):
//   Wd[k][m][qd] = dw[(qd * cw + m) * dkpad + k]                 (pack_conv rows n = qd * cw + o; one tap: column = packed channel k)
//   Wa[n][m][t]  = aw[n * akpad + k_index(cinw, 9, t, m)]        (conv_igemm_k_index)
// grid (ceil(Kc / 128), ceil(N / 128), 16 slots), 256 threads, 8 x 8 outputs each, 8-deep m tiles through LDS.
__device__ __forceinline__ int k_index_dev(int cin, int taps, int tap, int c) {   // conv_igemm_k_index (kernels_igemm.hip)
    const int full = cin / 32, cg = c / 32;
    const int g = cg < full ? cg * 4 * taps + tap * 4 + (c % 32) / 8 : full * 4 * taps + tap * ((cin % 32) / 8) + (c - full * 32) / 8;
    return g * 8 + (c % 8);
}

__global__ __launch_bounds__(256) void level6_compose_kernel(const Level6ComposeParams p) {
    __shared__ double As[8][128];   // [m][n]
    __shared__ double Bs[8][128];   // [m][k]
    const int tid = threadIdx.x;
    const int slot = blockIdx.z, cls = slot >> 2, a = (slot >> 1) & 1, b = slot & 1, py = cls >> 1, px = cls & 1;
    const int n0 = blockIdx.y * 128, k0 = blockIdx.x * 128;
    const int tk = tid & 15, tn = tid >> 4;
    double acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.0;
    const int an = n0 + (tid >> 1), ah = (tid & 1) * 4;   // Wa piece: row n, 4 consecutive m
    const int bm = tid >> 5, bk = k0 + (tid & 31) * 4;    // Wd piece: row m, 4 consecutive k
    for (int ky = 0; ky < 3; ++ky) {
        if ((((py + ky + 1) >> 1) - py) != a) continue;
        for (int kx = 0; kx < 3; ++kx) {
            if ((((px + kx + 1) >> 1) - px) != b) continue;
            const int t = ky * 3 + kx, qd = ((py + ky + 1) & 1) * 2 + ((px + kx + 1) & 1);
            for (int m0 = 0; m0 < p.dout; m0 += 8) {
                f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
                if (an < p.N) va = *reinterpret_cast<const f32x4*>(p.aw + (size_t)an * p.akpad + k_index_dev(p.cinw, 9, t, m0 + ah));
                if (bk < p.K) vb = *reinterpret_cast<const f32x4*>(p.dw + (size_t)(qd * p.cw + m0 + bm) * p.dkpad + bk);
                __syncthreads();
#pragma unroll
                for (int e = 0; e < 4; ++e) { As[ah + e][tid >> 1] = (double)va[e]; Bs[bm][(tid & 31) * 4 + e] = (double)vb[e]; }
                __syncthreads();
#pragma unroll
                for (int mm = 0; mm < 8; ++mm) {
                    double ar[8], br[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) { ar[i] = As[mm][tn * 8 + i]; br[i] = Bs[mm][tk * 8 + i]; }
#pragma unroll
                    for (int i = 0; i < 8; ++i)
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[i][j] = fma(ar[i], br[j], acc[i][j]);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int n = n0 + tn * 8 + i;
        if (n >= p.N) continue;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = k0 + tk * 8 + j;
            if (k < p.Kc) p.w2[((size_t)slot * p.N + n) * p.Kc + k] = acc[i][j];
        }
    }
}

// W2 (double) -> Winograd domain, rounded once: wc[class * P + u * NP + v][n][k] = sum_ab G[u][a] G[v][b] W2[class][a][b][n][k]
template <int M>
__global__ __launch_bounds__(256) void level6_filter_kernel(const Level6ComposeParams p) {
    using W = Wino<M>;
    constexpr int NP = W::NP;
    const size_t per = (size_t)p.N * p.Kc;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= per) return;
    const int cls = blockIdx.y;
    const int n = (int)(i / p.Kc), k = (int)(i - (size_t)n * p.Kc);
    double w[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) w[a][b] = p.w2[(size_t)(cls * 4 + a * 2 + b) * per + i];
#pragma unroll
    for (int u = 0; u < NP; ++u)
#pragma unroll
        for (int v = 0; v < NP; ++v) {
            double s = 0.0;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) s += W::g(u, a) * W::g(v, b) * w[a][b];
            p.wc[((size_t)(cls * NP * NP + u * NP + v) * p.Npad + n) * p.Kc + k] = (float)s;
        }
}

void launch_level6_compose(const Level6ComposeParams& p, hipStream_t s) {
    CCVPE_LAUNCH(level6_compose_kernel, dim3((p.Kc + 127) / 128, (p.N + 127) / 128, 16), dim3(256), 0, s, p);
    const size_t per = (size_t)p.N * p.Kc;
    const dim3 grid((unsigned)((per + 255) / 256), 4);
    if (p.wm == 4) CCVPE_LAUNCH(level6_filter_kernel<4>, grid, dim3(256), 0, s, p);
    else CCVPE_LAUNCH(level6_filter_kernel<2>, grid, dim3(256), 0, s, p);
}

}  // namespace ccvpe
