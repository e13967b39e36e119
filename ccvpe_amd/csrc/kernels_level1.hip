// Fused last decoder level:  ConvTranspose2d(k2,s2, CX->16) -> conv3x3(16->16)+ReLU -> conv3x3(16->{1,2})
// (-> F.normalize for the orientation branch), writing the NCHW outputs directly.
//
// Reference: deconv1 / conv1 (models.py:422-425, 625-626) and deconv1_ori / conv1_ori + normalize
// (models.py:443-446, 648-650); KITTI / Oxford copies at :727-728, :748-749, :1026-1028, :1046-1048.
//
// Unfused, this level moves three 512x512x16 fp32 tensors per sample through HBM and runs its 3x3 conv as
// an N=16 GEMM with 5 K tiles (prologue/epilogue dominated).  Here one workgroup owns a 16x16 output
// tile: the 10x10 input pixels it depends on are staged in LDS once.  Nothing lies between the transposed conv
// and the first 3x3 conv, so the two are composed into one convolution: a conv_a pixel of parity
// (py, px) reads a 2x2 window of input pixels with weights of its parity, so each of the four parity classes of
// the 18x18 conv_a tile is one [81 x 4 CX] x [4 CX x 16] GEMM whose A operand is gathered from the LDS tile at the
// four window shifts, on v_mfma_f32_16x16x4_f32 (host-composed weights, ccvpe_weights.hip; the transposed conv's bias
// enters through a 9-case border table).  The final 16->{1,2} conv runs as per-tap dot products on the same MFMAs
// plus nine adds per output, and only the 1-2 output channels leave the chip.  Zero padding of both 3x3 convs is
// applied where the reference applies it: intermediate pixels outside the 512x512 image are 0 (not bias).
#include "kernels.h"

#include <algorithm>
#include <cstdio>

namespace ccvpe {

typedef float f32x4 __attribute__((ext_vector_type(4)));

static constexpr int T = 16;          // output tile
static constexpr int AT = T + 2;      // conv_a-output tile (halo 1)
static constexpr int XT = T / 2 + 2;  // input tile (10 x 10)
static constexpr int PS = 20;         // floats per pixel in the P tile (18 + 2 pad)
static constexpr int NPOS = (AT / 2) * (AT / 2);    // conv_a pixels of one parity class: 9 x 9
static constexpr int NMT1 = (NPOS + 15) / 16;       // their m-tiles: 6
typedef float f32x2 __attribute__((ext_vector_type(2)));


#ifndef CCVPE_L1_CLOCK
#define CCVPE_L1_CLOCK 0   // dev builds (tools/build_variant.sh): 1 = every wave sums s_memtime per stage (input -> LDS + barrier, composed conv_a, tail products, barrier, tail conv + stores)
#endif
#if CCVPE_L1_CLOCK
__device__ unsigned long long g_l1_clk[10];
#define CCVPE_L1_STAMP(i_) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); clk[i_] += t_ - tprev; tprev = t_; }
#else
#define CCVPE_L1_STAMP(i_)
#endif

static constexpr int KCH_MAX = 4;     // input channels <= 64 (16 per chunk); the host falls back to the unfused path beyond
static constexpr int XI_MAX = (XT * XT * KCH_MAX * 4 + 255) / 256;   // float4 items per thread of one X tile

static constexpr int L1_WG_PER_CU = 2;   // persistent grid: workgroups per CU

// Persistent: L1_WG_PER_CU workgroups per CU loop over the 16x16 output tiles (XCD x owns a contiguous run, so neighbouring
// tiles - which share their input halo - meet in one L2).  Per-workgroup constants (the composed weights and the tail conv's
// weights as MFMA fragments, the interior bias, the per-lane LDS offsets) are set up once, and the next tile's input pixels are
// loaded into registers while the current tile runs its stages.  Measured before this: with one tile per workgroup 0.36 of the
// 1.06 ms was launch + weight staging + exposed load latency that nothing overlapped.
//
// NG, SCORE: the composed weights' shape (descriptor channel groups, score k-step) as compile-time constants for the input widths of
// the real variants (loc: score + 40 or 32 channels, ori: 32): a run-time group count costs a branch per group, around which the
// compiler moves all six accumulators between AGPRs and VGPRs.  NG == 0 is the generic form for any other width (run-time p.ng <= 16,
// p.score).
//
// The body (kernels_level1_tile.inc) is shared with the pose form (POSE: ccvpe_localize): one workgroup per sample runs the one tile that
// holds the sample's argmax (pose_index[blockIdx.x]) through the same stages - every value of that tile has the bits the persistent
// form computes for it - and the thread that owns the argmax pixel writes (cos, sin, angle_deg) to pose_rows[b][2..4] instead of storing the
// tile.  The fragment is included into both kernels rather than called as a force-inlined function: inlining reorders level1_kernel's
// kernarg loads and register assignment.
template <int COUT, int NG, int SCORE>
__global__ __launch_bounds__(256) void level1_kernel(const Level1Params p) {
    constexpr bool POSE = false;
    const int* pose_index = nullptr;
    float* pose_rows = nullptr;
    constexpr int pose_slot = 0, pose_sample = 0, pose_ld = 0, pose_r0 = 0;
#include "kernels_level1_tile.inc"
}

template <int COUT, int NG, int SCORE>
__global__ __launch_bounds__(256) void level1_pose_kernel(const Level1Params p, const int* pose_index, float* pose_rows) {
    constexpr bool POSE = true;
    const unsigned pose_slot = blockIdx.x;                 // one workgroup per sample: index[b], rows[b][0..4]
    const int pose_sample = (int)blockIdx.x;
    constexpr int pose_ld = 5, pose_r0 = 0;
#include "kernels_level1_tile.inc"
}

// Top-K pose plans (ccvpe_localize_topk): grid (K, B), workgroup (k, b) runs the tile of hypothesis index[b][k] and writes
// rows[b][k][2..4]; a slot without a peak (index -1) exits before it touches anything.  Two hypotheses in one tile each run it.
template <int COUT, int NG, int SCORE>
__global__ __launch_bounds__(256) void level1_topk_kernel(const Level1Params p, const int* pose_index, float* pose_rows) {
    constexpr bool POSE = true;
    const int K = (int)gridDim.x;
    const int pose_slot = (int)blockIdx.y * K + (int)blockIdx.x, pose_sample = (int)blockIdx.y;
    const int pose_ld = 5 * K, pose_r0 = 5 * (int)blockIdx.x;
    if (pose_index[pose_slot] < 0) return;
#include "kernels_level1_tile.inc"
}

bool level1_supported(int cxp) { return cxp >= 16 && cxp <= 16 * KCH_MAX && cxp % 16 == 0; }

size_t level1_lds_bytes(int cxp) {
    return ((size_t)XT * XT * (cxp + 4) + (size_t)AT * AT * PS) * sizeof(float);   // X tile, P tile
}

// shape class of the composed weights: f(NG, SCORE)
template <typename F>
static void with_shape(const Level1Params& p, F&& f) {
    using std::integral_constant;
    if (p.ng == 10 && p.score) f(integral_constant<int, 10>{}, integral_constant<int, 1>{});        // VIGOR / Oxford loc
    else if (p.ng == 8 && p.score) f(integral_constant<int, 8>{}, integral_constant<int, 1>{});     // KITTI loc
    else if (p.ng == 8 && !p.score) f(integral_constant<int, 8>{}, integral_constant<int, 0>{});    // ori
    else f(integral_constant<int, 0>{}, integral_constant<int, 0>{});
}

template <int COUT, int NG, int SCORE>
static void launch_level1_t(const Level1Params& p, dim3 grid, size_t lds, hipStream_t s) {
    static LdsAttr attr;
    ensure_dynamic_lds(attr, reinterpret_cast<const void*>(level1_kernel<COUT, NG, SCORE>), lds);
    CCVPE_LAUNCH((level1_kernel<COUT, NG, SCORE>), grid, dim3(256), lds, s, p);
}

void launch_level1(const Level1Params& p, hipStream_t s) {
    const size_t lds = level1_lds_bytes(p.cxp);
    const int tiles = (p.W / T) * (p.H / T) * p.B;
    dim3 grid(std::min(tiles, L1_WG_PER_CU * 256));   // persistent
#if CCVPE_L1_CLOCK
    static int calls = 0;
    const bool stamp = ++calls % 4 == 0;
    if (stamp) { (void)hipStreamSynchronize(s); unsigned long long z[10] = {}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_l1_clk), z, sizeof z); }
#endif
    if (p.cout == 1) with_shape(p, [&](auto ng, auto sc) { launch_level1_t<1, decltype(ng)::value, decltype(sc)::value>(p, grid, lds, s); });
    else with_shape(p, [&](auto ng, auto sc) { launch_level1_t<2, decltype(ng)::value, decltype(sc)::value>(p, grid, lds, s); });
#if CCVPE_L1_CLOCK
    if (stamp) {
        (void)hipStreamSynchronize(s);
        unsigned long long h[10];
        (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_l1_clk), sizeof h);
        double tot = 0;
        for (int i = 0; i < 5; ++i) tot += (double)h[i];
        std::fprintf(stderr, "level1<%d> cx %d: %.0f cycles/tile and wave: input->LDS+barrier %.0f %% conv_a %.0f %% tail products %.0f %% barrier %.0f %% tail conv %.0f %%\n",
                     p.cout, p.cx, tot / std::max(1.0, (double)h[8]), 100 * h[0] / tot, 100 * h[1] / tot, 100 * h[2] / tot, 100 * h[3] / tot, 100 * h[4] / tot);
    }
#endif
}

void launch_level1_pose(const Level1Params& p, const int* index, float* rows, hipStream_t s) {
    const size_t lds = level1_lds_bytes(p.cxp);
    with_shape(p, [&](auto ng, auto sc) {
        constexpr int NG = decltype(ng)::value, SCORE = decltype(sc)::value;
        static LdsAttr attr;
        ensure_dynamic_lds(attr, reinterpret_cast<const void*>(level1_pose_kernel<2, NG, SCORE>), lds);
        CCVPE_LAUNCH((level1_pose_kernel<2, NG, SCORE>), dim3(p.B), dim3(256), lds, s, p, index, rows);
    });
}

void launch_level1_topk(const Level1Params& p, const int* index, int k, float* rows, hipStream_t s) {
    const size_t lds = level1_lds_bytes(p.cxp);
    with_shape(p, [&](auto ng, auto sc) {
        constexpr int NG = decltype(ng)::value, SCORE = decltype(sc)::value;
        static LdsAttr attr;
        ensure_dynamic_lds(attr, reinterpret_cast<const void*>(level1_topk_kernel<2, NG, SCORE>), lds);
        CCVPE_LAUNCH((level1_topk_kernel<2, NG, SCORE>), dim3(k, p.B), dim3(256), lds, s, p, index, rows);
    });
}

}  // namespace ccvpe
