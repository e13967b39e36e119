// Fused last decoder level:  ConvTranspose2d(k2,s2, CX->16) -> conv3x3(16->16)+ReLU -> conv3x3(16->{1,2})
// (-> F.normalize for the orientation branch), writing the NCHW outputs directly.
//
// Reference: deconv1 / conv1 (models.py:422-425, 625-626) and deconv1_ori / conv1_ori + normalize
// (models.py:443-446, 648-650); KITTI / Oxford copies at :727-728, :748-749, :1026-1028, :1046-1048.
//
// Unfused, this level moves three 512x512x16 fp32 tensors per sample through HBM and runs its 3x3 conv as
// an N=16 GEMM with 5 K tiles (prologue/epilogue dominated).  Here one workgroup owns a 16x16 output
// tile (below; a 32x16 tile - L1Shape - has the same stages on larger extents): the 10x10 input pixels it depends on are staged in LDS once.  Nothing lies between the transposed conv
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

typedef float f32x2 __attribute__((ext_vector_type(2)));

// Output tile (TY rows x TX columns) and workgroup size of the shared body (kernels_level1_tile.inc), by Level1Params::tile.
// 16 x 16: an 18 x 18 conv_a tile for 256 outputs and 4 x 6 m-tiles for 4 x 81 positions - 384 GEMM rows per 256 outputs.
// 32 x 16: 18 x 34 for 512 and 4 x 10 m-tiles for 4 x 153 positions - 640 rows per 512 outputs, 1/6 fewer MFMAs per output.
template <int TILE> struct L1Shape;
template <> struct L1Shape<0> { static constexpr int TY = 16, TX = 16, NTHR = 256; };
template <> struct L1Shape<1> { static constexpr int TY = 16, TX = 32, NTHR = 512; };   // wave = (parity class, half of its m-tiles)
static constexpr int L1_TILES = 2;
// Floats per pixel of the P tile.  16 wide: 18 + 2 pad.  32 wide: the 9 COUT real columns and no more - two loc workgroups fit a CU's LDS,
// and stage 3's reads (32 consecutive pixels per LDS lane group) are conflict-free: dword reads at stride 9, 8-byte reads at stride 18.
static constexpr int l1_ps(int cout, int tx) { return tx == 16 ? 20 : 9 * cout; }


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

static constexpr int L1_WAVES_PER_CU = 8;   // persistent grid: two 256-thread workgroups or one 512-thread workgroup per CU

// Persistent: L1_WAVES_PER_CU waves per CU loop over the output tiles (XCD x owns a contiguous run, so neighbouring
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
template <int COUT, int NG, int SCORE, int TILE>
__global__ __launch_bounds__(L1Shape<TILE>::NTHR) void level1_kernel(const Level1Params p) {
    constexpr bool POSE = false;
    const int* pose_index = nullptr;
    float* pose_rows = nullptr;
    constexpr int pose_slot = 0, pose_sample = 0, pose_ld = 0, pose_r0 = 0;
#include "kernels_level1_tile.inc"
}

// (the pose and top-K forms run one tile per workgroup and stay on 16 x 16: fewer pixels computed around the one that is kept)
template <int COUT, int NG, int SCORE>
__global__ __launch_bounds__(256) void level1_pose_kernel(const Level1Params p, const int* pose_index, float* pose_rows) {
    constexpr bool POSE = true;
    constexpr int TILE = 0;
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
    constexpr int TILE = 0;
    const int K = (int)gridDim.x;
    const int pose_slot = (int)blockIdx.y * K + (int)blockIdx.x, pose_sample = (int)blockIdx.y;
    const int pose_ld = 5 * K, pose_r0 = 5 * (int)blockIdx.x;
    if (pose_index[pose_slot] < 0) return;
#include "kernels_level1_tile.inc"
}

bool level1_supported(int cxp) { return cxp >= 16 && cxp <= 16 * KCH_MAX && cxp % 16 == 0; }

template <int TILE>
static size_t lds_bytes(int cxp, int cout) {
    using S = L1Shape<TILE>;
    return ((size_t)(S::TY / 2 + 2) * (S::TX / 2 + 2) * (cxp + 4) + (size_t)(S::TY + 2) * (S::TX + 2) * l1_ps(cout, S::TX)) * sizeof(float);   // X tile, P tile
}

int level1_tile(const Level1Params& p) {
    const int t = p.tile < 0 || p.tile >= L1_TILES ? 0 : p.tile;
    return t == 1 && (p.H % L1Shape<1>::TY || p.W % L1Shape<1>::TX) ? 0 : t;
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

template <int COUT, int NG, int SCORE, int TILE>
static void launch_level1_t(const Level1Params& p, hipStream_t s) {
    using S = L1Shape<TILE>;
    const size_t lds = lds_bytes<TILE>(p.cxp, COUT);
    const int tiles = (p.W / S::TX) * (p.H / S::TY) * p.B;
    dim3 grid(std::min(tiles, p.max_wg >= 8 ? p.max_wg : L1_WAVES_PER_CU * 64 / S::NTHR * 256));   // persistent
    static LdsAttr attr;
    ensure_dynamic_lds(attr, reinterpret_cast<const void*>(level1_kernel<COUT, NG, SCORE, TILE>), lds);
    CCVPE_LAUNCH((level1_kernel<COUT, NG, SCORE, TILE>), grid, dim3(S::NTHR), lds, s, p);
}

template <int COUT>
static void launch_level1_c(const Level1Params& p, hipStream_t s) {
    with_shape(p, [&](auto ng, auto sc) {
        constexpr int NG = decltype(ng)::value, SCORE = decltype(sc)::value;
        if (level1_tile(p) == 1) launch_level1_t<COUT, NG, SCORE, 1>(p, s);
        else launch_level1_t<COUT, NG, SCORE, 0>(p, s);
    });
}

void launch_level1(const Level1Params& p, hipStream_t s) {
#if CCVPE_L1_CLOCK
    static int calls = 0;
    const bool stamp = ++calls % 4 == 0;
    if (stamp) { (void)hipStreamSynchronize(s); unsigned long long z[10] = {}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_l1_clk), z, sizeof z); }
#endif
    if (p.cout == 1) launch_level1_c<1>(p, s);
    else launch_level1_c<2>(p, s);
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
    const size_t lds = lds_bytes<0>(p.cxp, 2);
    with_shape(p, [&](auto ng, auto sc) {
        constexpr int NG = decltype(ng)::value, SCORE = decltype(sc)::value;
        static LdsAttr attr;
        ensure_dynamic_lds(attr, reinterpret_cast<const void*>(level1_pose_kernel<2, NG, SCORE>), lds);
        CCVPE_LAUNCH((level1_pose_kernel<2, NG, SCORE>), dim3(p.B), dim3(256), lds, s, p, index, rows);
    });
}

void launch_level1_topk(const Level1Params& p, const int* index, int k, float* rows, hipStream_t s) {
    const size_t lds = lds_bytes<0>(p.cxp, 2);
    with_shape(p, [&](auto ng, auto sc) {
        constexpr int NG = decltype(ng)::value, SCORE = decltype(sc)::value;
        static LdsAttr attr;
        ensure_dynamic_lds(attr, reinterpret_cast<const void*>(level1_topk_kernel<2, NG, SCORE>), lds);
        CCVPE_LAUNCH((level1_topk_kernel<2, NG, SCORE>), dim3(k, p.B), dim3(256), lds, s, p, index, rows);
    });
}

}  // namespace ccvpe
