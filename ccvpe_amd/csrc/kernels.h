// Internal kernel interface of libccvpe_hip.so (gfx950 only).  All activations are fp32 NHWC.
#pragma once
#include <functional>
#include <vector>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ticket.h"

namespace ccvpe {

// Every kernel launch of the library goes through this macro: ccvpe_launch_count() (include/ccvpe.h) lets a caller count the launches of
// a forward call - the batch-1 latency record of bench.py reports launches per frame.
extern thread_local unsigned long long g_launches;
#define CCVPE_LAUNCH(...) do { ++::ccvpe::g_launches; hipLaunchKernelGGL(__VA_ARGS__); } while (0)

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: the launchers raise it lazily, once per
// (kernel instantiation, device) - a process may hold handles on several devices.  `state` is a function-local static array
// (one slot per device ordinal); a failing hipFuncSetAttribute leaves the slot unset, the launch that follows then fails and
// the forward call reports it through hipGetLastError.
struct LdsAttr { size_t set[16] = {0}; };
inline void ensure_dynamic_lds(LdsAttr& state, const void* kernel, size_t bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = 0;
    if (bytes > state.set[dev] && hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess) state.set[dev] = bytes;
}

enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_SWISH = 2 };

// A destination view of an NHWC tensor: element (pixel p, channel c) lives at ptr[p*ld + coff + c].
struct Dst {
    float* ptr;
    int ld;
    int coff;
    // split != 0: the tensor is stored as two bf16 planes (bf16x3 mode): hi at ptr, lo `plane` bf16 elements later
    int split;
    long long plane;
};

// ---------------------------------------------------------------------------------------------
// Implicit-GEMM convolution on fp32 MFMA (v_mfma_f32_32x32x2_f32).
//   out[m, n] = act( sum_k A[m, k] * Wp[n, k] + bias[n] ) (+ resid[m, n])
// m = output pixel (b, oy, ox) for MODE_CONV, input pixel for MODE_DECONV (k2 s2 transposed conv,
// n = (dy*2+dx)*cout + o, pixel-shuffled on store).  k = (ky*KW + kx)*Cin + c, Cin % 8 == 0.
// ---------------------------------------------------------------------------------------------
enum { MODE_CONV = 0, MODE_DECONV = 1 };

struct ConvParams {
    const float* in;
    int in_ld;                 // floats per input pixel (>= Cin)
    int B, H, W, Cin;          // input geometry
    int OH, OW;                // GEMM-row geometry (conv: output map; deconv: == H, W)
    int KH, KW, stride, pad_t, pad_l;
    const float* wpk;          // [Npad][Kpad], k contiguous
    const unsigned short* w_hi;   // bf16x3 mode: bf16(w) and bf16(w - hi), same [Npad][Kpad] layout (null = unavailable)
    const unsigned short* w_lo;
    int Kpad;                  // multiple of 32
    int Npad;                  // rows in wpk (multiple of conv_igemm_npad())
    int nchunks;               // KH*KW*Cin/8 valid 8-channel chunks
    const float* bias;         // [N]
    int N;
    int act;
    const float* gate;         // optional [B][Cin] multiplier on A (squeeze-excite), 1x1 only
    const float* resid;        // optional residual [M][resid_ld]
    int resid_ld;
    Dst dst[3];
    int ndst;
    int mode;
    int deconv_cout;
    int M;                     // B*OH*OW
    unsigned in_bytes;         // extent of `in` for the bounds-checked buffer loads (< 2 GiB)
    int in_split;              // input is a split bf16 tensor (hi plane | lo plane); bf16x3 tiles only
    unsigned in_plane_bytes;   // byte distance between the two planes
    unsigned w_plane_bytes;    // extent of one bf16 weight plane (Npad*Kpad*2)
    unsigned gate_bytes;
    // filled by launch_conv_igemm (conv_igemm_prepare): K-order arithmetic, see chunk_to_tap()
    int taps4;                 // 4 * KH*KW
    int kfull_chunks;          // chunks covered by whole 32-channel groups = (Cin/32) * 4 * taps
    int kfull_c0;              // (Cin/32)*32: first channel of the partial group
    int knc;                   // chunks per tap in the partial group (Cin%32)/8
    int div_4t_mul;            // g / taps4      == (g * mul) >> 20
    int div_nc_mul;            // idx / knc      == (idx * mul) >> 8
    int div_kw_mul;            // tap / KW       == (tap * mul) >> 5
    int vec_epi;               // filled by launch_conv_igemm: 16-byte epilogue stores are legal
    int splitk;                // filled by launch_conv_igemm from the cfg word: K split over gridDim.z
    float* partial;            // split-K slab scratch [splitk][M][N] (null = split-K unavailable)
    size_t partial_floats;
    // Self-reducing split-K (round 4, ticket.h): the K slices of an output region draw tickets on tickets[region]; the last one sums the
    // slabs in slice order and runs the epilogue itself - no splitk_reduce_kernel launch.  Chosen per launch by the cfg word (split code
    // 64 + S); needs `tickets` (>= CONV_TICKETS counters, zero between launches).
    unsigned* tickets;
    int split_fused;           // filled by launch_conv_igemm
    // exact division by W and H for the transposed-conv pixel shuffle (filled by conv_igemm_prepare): q = (umulhi(n, mul) + n) >> shift
    unsigned fdw_mul, fdw_shift, fdh_mul, fdh_shift;
    // Winograd F(2x2,3x3) form of a 3x3 / stride 1 / pad 1 layer (kernels_wino.hip); null = not packed
    const float* wino_w;       // [Cin/8][16][wino_n16][128]
    int wino_n16;              // ceil(N / 16)
    int wino_nb, wino_n16_off; // F(4x4) sub-launches: n-blocks this launch covers (0 = all), first 16-channel slice
    unsigned wino_bytes;
    // Winograd F(4x4,3x3) form (kernels_wino4.hip), packed for the wide decoder layers only; null = not packed
    const float* wino4_w;      // [ceil(Cin/16)*4 k-steps][9 xi quads][wino_n16][64 lanes][4]
    unsigned wino4_bytes;
    // xi-split F(4x4) form for layers of <= 128 output channels (kernels_wino4x.hip); null = not packed
    const float* wino4x_w;     // [k-step][wave][16-byte load][64 lanes][4]
    unsigned wino4x_bytes;
    int wino4x_cfg;            // configuration index the weights were packed for (conv_wino4x_config(N))
    // deep-K / narrow-N project GEMM (kernels_proj.hip): the 1x1 weights in MFMA fragment order, null = not packed
    const float* proj_w;       // [Cin / 16 steps][ceil(N / 16) column tiles][64 lanes][4]
    unsigned proj_bytes;
    // Squeeze-excite in the prologue of the latency-form project GEMM (kernels_proj.hip, batch <= 4; model.py:113-118): instead of a gate
    // vector the launch gets the fused front kernel's per-item squeeze rows (ticket.h: SeTicket::sqpart) and the excite weights, and
    // every wave computes the gates of ITS K slice while its operands are in flight.  se_rows == null: `gate` as usual.
    const float* se_rows;      // [B][se_nrows][se_sq]
    int se_nrows, se_sq;
    float se_inv_hw;
    const float* se_b1;        // [SQ]
    const float* se_w2;        // [SQ][Cin]
    const float* se_b2;        // [Cin]
};

// One descriptor per tiled convolution kernel.  Every family file keeps its array beside its launchers (conv_*_tiles) and
// kernels_igemm.hip concatenates them once, in the order igemm, bf16x3, wino, pw: tile id = index + 1, 0 picks from (M, N).
// A launch cfg word is tile | (split code << 8).
enum { TILE_AUTO = 0 };
enum TileFamily { TILE_IGEMM, TILE_BF16X3, TILE_WINO, TILE_PW };
using ConvLaunch = void (*)(const ConvParams&, hipStream_t);
struct ConvTile {
    int bm, bn;                // output pixels / channels per workgroup (padding of M and N)
    const char* name;
    ConvLaunch launch;
    TileFamily family;
    double intrinsic = 0.0;    // prior of the shape heuristic (pick_tile); 0: only a tuning table or the autotuner names the tile
    int wino_f = 0;            // Winograd output tile edge, 2 or 4
    int xcfg = -1;             // >= 0: xi-split F(4x4) configuration (kernels_wino4x.hip)
    int proj_rt = 0;           // > 0: a kernels_proj.hip tile of that many row tiles; >= 100: its latency form
};
// one constructor per family: a table row names only what its family has
constexpr ConvTile igemm_tile(int bm, int bn, const char* name, ConvLaunch l, double intrinsic) { return {bm, bn, name, l, TILE_IGEMM, intrinsic}; }
constexpr ConvTile bf16x3_tile(int bm, int bn, const char* name, ConvLaunch l) { return {bm, bn, name, l, TILE_BF16X3}; }
constexpr ConvTile wino_tile(int bm, int bn, const char* name, ConvLaunch l, int f, int xcfg = -1) { return {bm, bn, name, l, TILE_WINO, 0.0, f, xcfg}; }
constexpr ConvTile pw_tile(int bm, int bn, const char* name, ConvLaunch l, int proj_rt = 0) { return {bm, bn, name, l, TILE_PW, 0.0, 0, -1, proj_rt}; }
static constexpr int CONV_TICKETS = 8192;   // ticket counters a convolution launch may use (output regions of a split-K launch)
static constexpr int SPLIT_FUSED = 64;       // split code 64 + S: S slices, reduced by the last arriver (S <= 32)
int conv_num_tiles();
const ConvTile* conv_tile(int id);           // by tile id or cfg word (masks & 0xff); null for 0 and ids past the last
const char* conv_tile_name(int id);          // "" where conv_tile is null
int conv_proj_lat_tile();                    // id of conv_projl_1: the one kernel that computes squeeze-excite gates itself
bool conv_tile_runs(const ConvTile& t, const ConvParams& p);   // the form the tile needs is packed and the layer is shaped for it
// the split codes a tile takes beyond a plain K split with the reduce launch: self-reducing (SPLIT_FUSED + S), the F(4x4) tail split (255).
// The pointwise family (TILE_PW) keeps K whole; its latency form splits it only self-reducing.
enum { SPLIT_SELF = 1, SPLIT_TAIL = 2 };
int conv_tile_splits(const ConvTile& t);
double conv_tile_util(const ConvParams& p, const ConvTile& t);
long long conv_tile_blocks(const ConvParams& p, const ConvTile& t);
int conv_tile_last();        // cfg word of the most recent launch on this thread (then reset to 0)
void conv_tile_note_unfused();   // called by a launcher that drops the self-reducing form of the split it was handed
int conv_igemm_prepare(ConvParams& p);
int conv_igemm_k_index(int cin, int taps, int tap, int c);   // packed-weight column of (tap, channel)
int launch_conv_igemm(const ConvParams& p, int tile, hipStream_t s);   // 0, or -1 for unsupported geometry
int conv_igemm_npad();       // row padding of packed weights (multiple every tile divides)
void launch_splitk_reduce(const ConvParams& p, hipStream_t s);
const ConvTile* conv_bf16x3_tiles(int* n);
const ConvTile* conv_wino_tiles(int* n);
bool conv_wino_supported(const ConvParams& p);
bool conv_wino4_supported(const ConvParams& p);
void launch_wino4_64(const ConvParams& p, hipStream_t s);
void launch_wino4_128(const ConvParams& p, hipStream_t s);
bool conv_wino4_tail_applied();
void launch_wino4x(const ConvParams& p, hipStream_t s);       // xi-split form (kernels_wino4x.hip)
bool conv_wino4x_supported(const ConvParams& p);
int conv_wino4x_config(int N);
size_t conv_wino4x_pack(int N, int cin, const std::function<float(int, int, int)>& get, std::vector<float>& out, int* cfg_out);
size_t conv_wino4_pack(int N, int cin, const std::function<float(int, int, int)>& get, std::vector<float>& out);
size_t conv_wino_pack(int N, int cin, const std::function<float(int, int, int)>& get, std::vector<float>& out, int* n16_out);
// pointwise persistent kernel (kernels_pw.hip): 1x1 convs / k2s2 transposed convs with K <= 512
const ConvTile* conv_pw_tiles(int* n);
bool conv_pw_supported(const ConvParams& p);
bool conv_pw_fits(int bn, int kpad);
// deep-K project GEMM (kernels_proj.hip)
bool conv_proj_supported(const ConvParams& p, int rt);
void launch_proj(const ConvParams& p, int rt, hipStream_t s);
bool conv_proj_wanted(int N, int cin);
size_t conv_proj_pack(int N, int cin, const std::function<float(int, int)>& get, std::vector<float>& out, int taps = 1);
bool conv_proj_lat_wanted(int taps, int KH, int KW, int cinp);   // deep-K 1x1 / k2s2 layers the latency form may serve

// ---------------------------------------------------------------------------------------------
// Encoder pieces
// ---------------------------------------------------------------------------------------------
struct StemParams {
    const float* in;           // NCHW [B,3,H,W]
    int B, H, W, OH, OW;
    int pad_t, pad_l;
    int circular;
    const float* w;            // [27][32]  k = (c*3+ky)*3+kx, BN folded
    const float* bias;         // [32]
    float* out;                // NHWC [B,OH,OW,32]
};
void launch_stem(const StemParams& p, hipStream_t s);

// Stem + block 0's depthwise conv in one launch (block 0 has no expand conv: its depthwise conv reads the stem output directly)
struct StemDwParams {
    StemParams st;             // st.out unused
    const float* wd;           // [9][32] depthwise taps, BN folded
    const float* bd;           // [32]
    float* out;                // NHWC [B,OH,OW,32]: swish(dw(swish(stem)))
    float* pool_partial;       // [B][S][32] partial sums of `out`, S = stem_dw_tiles
    SeTicket se;               // se.counter != null: the workgroup that finishes a sample last runs its squeeze-excite (ticket.h)
};
int stem_dw_tiles(int OH, int OW);   // pooling partial rows per sample
void launch_stem_dw(const StemDwParams& p, hipStream_t s);

struct DwParams {
    const float* in;           // NHWC [B,H,W,C]
    int B, H, W, C, OH, OW;
    int k, stride, pad_t, pad_l, circular;
    const float* w;            // [k*k][C], BN folded
    const float* bias;         // [C]
    float* out;                // NHWC [B,OH,OW,C], swish applied
    float* pool_partial;       // [B][S][C] partial sums of `out` for squeeze-excite
    int S;                     // strip lanes per sample
    SeTicket se;               // se.counter != null: squeeze-excite by the last-arriving workgroup of a sample (ticket.h)
};
void launch_depthwise(const DwParams& p, hipStream_t s);
int depthwise_strip_lanes(int B, int OH, int OW, int C, int k, int stride);

// Fused expand (1x1 + BN + swish) + depthwise (k x k + BN + swish) + SE pooling partials (kernels_mbconv.hip)
struct MbFrontParams {
    const float* x;            // NHWC [B,H,W,Cin]
    int B, H, W, Cin, cinp;    // cinp = Cin rounded up to 16 (weights zero padded)
    int mid;                   // expanded channels, multiple of 48
    const float* we;           // [mid][cinp], BN folded
    const float* be;           // [mid]
    const float* wd;           // [k*k][mid], BN folded
    const float* bd;           // [mid]
    int k, s, pad_t, pad_l, circular, OH, OW;
    float* out;                // NHWC [B,OH,OW,mid]
    float* pool;               // [B][tiles][mid]
    SeTicket se;               // se.counter != null: squeeze-excite by the last-arriving workgroup of a sample (ticket.h); the kernels
                               // that take it are named by the *_ticket_rows functions below (0 = this launch cannot)
    int spread;                // latency plans: work items a launch may spread to by cutting its work finer (more strips of the image-resident
                               // form, channel ranges per tile group of the wave form); 0 = never.  Set by the plan (CCVPE_FRONT_SPREAD, default 128)
};
void launch_mbconv_front(const MbFrontParams& p, hipStream_t s);
int mbconv_front_tiles(int k, int s, int OH, int OW);
// pooling partial rows per sample when the launch runs with a ticket (the wave-local form then pre-reduces four tiles per workgroup);
// 0 = the kernel launch_mbconv_front / launch_mbconv_image would pick for these parameters does not take a ticket
int mbconv_front_ticket_rows(const MbFrontParams& p);
int mbconv_image_ticket_rows(const MbFrontParams& p);
int mbconv_front_ticket_split(const MbFrontParams& p);   // workgroups per tile group of the wave form (channel ranges): tickets per row
bool mbconv_front_supported(int k, int s, int cin, int mid);
bool mbconv_front_profitable(int k);
// image-resident form (kernels_mbimg.hip): the whole image, or horizontal strips of it, per 16-channel chunk in LDS
bool mbconv_image_supported(const MbFrontParams& p);
int mbconv_image_strips(const MbFrontParams& p);   // pooling partial rows per sample ([B][strips][mid])
void launch_mbconv_image(const MbFrontParams& p, hipStream_t s);

struct SeParams {
    const float* pool_partial; // [B][S][C]
    int B, S, C, SQ;
    float inv_hw;
    const float* w1;           // [SQ][C]
    const float* b1;           // [SQ]
    const float* w2;           // [SQ][C] (transposed at pack time)
    const float* b2;           // [C]
    float* gate;               // [B][C] sigmoid(...)
    float* pooled;             // [B][SC][C] scratch: second-stage partial sums
    int SC;                    // second-stage split of the S partial rows (<= 16)
    float* sq;                 // [B][SQ] scratch: squeezed activations
};
void launch_se(const SeParams& p, hipStream_t s);

// ground descriptor: d_k[b][w*c_k + ch] = b2_k + sum_h wh_k[h] * Y[b,h,w,off_k+ch]
struct GrdDescParams {
    const float* y;            // NHWC [B,Hf,Wf,Ntot] (1x1 conv output incl. bias)
    int B, Hf, Wf, Ntot;
    int nlev;
    int c[6], off[6];          // per level head width and channel offset in y
    const float* wh[6];        // [Hf]
    float b2[6];
    float* desc;               // [B][Ltot] levels back to back
    int loff[6];               // element offset of level k inside a sample's row
    int Ltot;
};
void launch_grd_desc(const GrdDescParams& p, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Rolling match + L2 normalise + concat
// ---------------------------------------------------------------------------------------------
struct MatchParams {
    const float* x;            // NHWC [B,HW,C] (ld = x_ld)
    int x_ld;
    int B, HW, C;
    const float* g;            // [B][g_ld] descriptor, first L used
    int g_ld, L;
    int R;
    int shift[32];             // window_r[c] = x[(c + shift[r]) mod C]
    uint32_t inmax;            // rolls that take part in the max
    float* ms;                 // NCHW [B,R,HW] or null
    // loc concat buffer: ch0 = max, ch1..7 = 0, ch 8.. = normalised x
    float* cat_max;  int cat_max_ld;
    // ori concat buffer: ch0..R-1 = scores, zero pad to rpad, then normalised x
    float* cat_all;  int cat_all_ld;  int rpad;
    int P;                     // pixels per block (power of two, divides HW)
    float* gg_scratch;         // [B][match_scratch_floats(C)]: rolled descriptor of the small-C register form / Gm, Mk of the MFMA form (null = LDS form only)
    int prep_done;             // 1: launch_match_prep already ran on these parameters (launch_match then skips its preparation launch)
    int no_wide;               // 1: never the latency forms (sixteen waves per workgroup / four waves per 64 pixels) - CCVPE_MATCH_WIDE=0, read per plan
};
void launch_match(const MatchParams& p, hipStream_t s);
// The preparation launch alone (rolled descriptor / Gm, Mk into gg_scratch): it depends on the ground descriptor only, so a plan may issue it
// long before the aerial features exist.  Same form decision as launch_match when given the same parameters; no launch for the LDS form.
void launch_match_prep(const MatchParams& p, hipStream_t s);
void launch_match_prep_all(const MatchParams* ps, int n, hipStream_t s);   // the preparation of up to six levels in one launch
int match_pixels_per_block(int HW, int C);
size_t match_scratch_floats(int C);   // per-sample floats of MatchParams::gg_scratch

// ---------------------------------------------------------------------------------------------
// Tail: 16 -> {1,2} 3x3 conv to NCHW (+ unit-normalise for ori), softmax, post-processing
// ---------------------------------------------------------------------------------------------
struct TailConvParams {
    const float* in;           // NHWC [B,H,W,16]
    int B, H, W;
    const float* w;            // [9][16][cout]
    float bias[2];
    int cout;                  // 1 or 2
    int normalize;             // L2 normalise over the cout channels (F.normalize, eps 1e-12)
    float* out;                // NCHW [B,cout,H,W]
    float* raw;                // optional NCHW un-normalised copy (debug tap) or null
};
void launch_tail_conv(const TailConvParams& p, hipStream_t s);

// Fused last decoder level (kernels_level1.hip): deconv k2s2 (cx -> 16) + conv3x3 (16 -> 16) (composed into one conv) + ReLU +
// conv3x3 (16 -> cout) [+ L2 normalise], NHWC input at H/2 x W/2, NCHW output at H x W.
struct Level1Params {
    const float* x;            // NHWC [B, H/2, W/2, x_ld], first cx channels used
    int x_ld, cx, cxp;         // cxp = cx rounded up to 16 (the X tile's channel count)
    int B, H, W;               // output geometry (512 x 512)
    // transposed conv composed with the first 3x3 conv (ccvpe_weights.hip): K = the score channel at the 4 window positions (if
    // score) + ng groups of 4 descriptor channels (input channels c0 + 4g .. + 3) at the 4 window positions
    int c0, ng, score;
    const float* wc;           // [4 parity][ng][64 lane][4]: lane = window (lane >> 4) x output channel (lane & 15)
    const float* ws;           // [4 parity][64 lane] the score channel's k-step (null without a score channel)
    const float* bc;           // [9][16] conv_a bias by border case (3 * row case + column case; 0 interior, 1 first, 2 last)
    const float* wt;           // [9][cout][16]
    float bt[2];
    int cout, normalize;
    float* out;                // NCHW [B, cout, H, W]
    float* raw;                // optional un-normalised copy (debug tap)
    int tile;                  // output tile of launch_level1: 0 = 16 x 16, 1 = 32 wide x 16 high (where W % 32 == 0; else 16 x 16)
    int max_wg;                // 0: the persistent grid; else at most this many workgroups (>= 8: one per XCD), so that a small
                               // problem still loops over tiles (ccvpe_op_level1)
};
void launch_level1(const Level1Params& p, hipStream_t s);
int level1_tile(const Level1Params& p);   // the tile launch_level1 runs for p
bool level1_supported(int cxp);   // input channel count the fused kernel takes
// Pose plans (ccvpe_localize): the same fused level for ONE 16 x 16 tile per sample - the tile holding index[b] (pose_argmax_kernel) -
// one workgroup per sample; the thread that owns the argmax pixel writes rows[b][2..4] = (cos, sin, angle_deg).  cout 2, normalize 1.
void launch_level1_pose(const Level1Params& p, const int* index, float* rows, hipStream_t s);
// Top-K pose plans: grid (k, B), workgroup (j, b) runs the tile of index[b][j] and writes rows[b][j][2..4]; index -1 exits at once.
void launch_level1_topk(const Level1Params& p, const int* index, int k, float* rows, hipStream_t s);

// Composed decoder level 6 (kernels_level6.hip): deconv6 composed into the 1024-channel half of conv6.0, per output
// parity class a 2x2-tap convolution on the 8x8 grid, run as Winograd F(wm x wm, 2x2): P = (wm + 1)^2 positions, 4 P groups.
struct Level6Params {
    int wm;                    // Winograd output tile edge: 4 (25 positions) or 2 (9 positions)
    int B;
    int K, Kc;                 // floats per input pixel (score pad + descriptor channels, multiple of 4); K rounded up to 32
    int N, Npad;               // conv6.0's output channels (multiple of 4); rows of a weight panel (N rounded up to 128, zero rows)
    int R, bm;                 // rows of a group = level6_rows(B, wm, &bm): B (8 / wm)^2 tiles, zero rows up to the GEMM's tile height bm
    int groups;                // groups of the GEMM launch: 4 P composed, 36 for a split-form 3x3 layer (Split6Params)
    const float* x;            // NHWC [B, 8, 8, K]
    float* v;                  // [4 P][R][Kc] transformed input
    const float* wc;           // [4 P][Npad][Kc] composed weights in the Winograd domain
    float* mp;                 // [4 P][R][N] products
    const float* skip;         // NHWC [B, 16, 16, N]: the skip half of conv6.0 (no bias, no activation)
    const float* bc;           // [9][N] conv6.0's bias + the transposed conv's bias through the in-image taps, by border case
                               // (3 * row case + column case; 0 interior, 1 first, 2 last)
    float* out;                // NHWC [B, 16, 16, N] = ReLU(conv6.0(cat[deconv6(x), skip input]))
};
int level6_positions(int wm);
int level6_rows(int B, int wm, int* bm_out);
bool level6_supported(const Level6Params& p);   // sizes only (pointers are not looked at)
void launch_level6_transform(const Level6Params& p, hipStream_t s);
void launch_level6_gemm(const Level6Params& p, hipStream_t s);
void launch_level6_combine(const Level6Params& p, hipStream_t s);
// the composed weights from the two layers' packed fp32 weights, in double, rounded once (two launches; `w2` is the scratch between them)
struct Level6ComposeParams {
    int wm;
    const float* dw;           // transposed conv, pack_conv layout [4 cw rows (qd * cw + m)][dkpad], column = packed input channel
    int cw, dout, dkpad;       // row pitch of a (dy, dx) group, real output channels (multiple of 8), row length
    const float* aw;           // conv6.0, pack_conv layout [n][akpad], column = conv_igemm_k_index(cinw, 9, tap, channel)
    int cinw, akpad;
    int K, Kc, N, Npad;        // as Level6Params
    double* w2;                // [16 = class * 4 + window][N][Kc]
    float* wc;                 // [4 P][Npad][Kc], rows N .. Npad zero before the launch
};
void launch_level6_compose(const Level6ComposeParams& p, hipStream_t s);

// A 3x3 layer (pad 1) on the 16 x 16 level-6 map in split Winograd form F(4x4,3x3), on the same grouped GEMM:
//   split6_transform   x -> V[36 positions][R rows = tiles of all samples][Kc]          (B^T d B, kernels_wino4.hip's matrices)
//   level6_gemm        M'[xi] = V[xi] . Wc[xi]^T, 36 groups (split6_gemm_params)
//   split6_inverse     A^T M' A per (tile, 4 channels) (+ bias, ReLU) -> the layer's output pixels
struct Split6Params {
    int B, C, Kc;              // samples; input channels (multiple of 4); C rounded up to 32 (zero channels)
    int N, Npad;               // output channels (multiple of 4); rows of a weight panel (N rounded up to 128)
    int R, bm;                 // rows of a position = split6_rows(B, &bm): 16 B tiles, zero rows up to the GEMM's tile height bm
    const float* x;            // NHWC [B, 16, 16, .]: pixel (b, y, x), channel c at x[((b * 16 + y) * 16 + x) * x_ld + x_coff + c]
    int x_ld, x_coff;          // (multiples of 4)
    float* v;                  // [36][R][Kc]
    const float* wc;           // [36][Npad][Kc]: G g G^T per (output, input) channel, xi = 6 r + q (split6_pack_weights)
    float* mp;                 // [36][R][N]
    const float* bias;         // [N], or null: no bias
    int relu;
    float* out;                // NHWC, out[((b * 16 + y) * 16 + x) * out_ld + out_coff + n]
    int out_ld, out_coff;      // (multiples of 4)
};
int split6_rows(int B, int* bm_out);
bool split6_supported(const Split6Params& p);   // sizes only (pointers are not looked at)
Level6Params split6_gemm_params(const Split6Params& p);
void launch_split6_transform(const Split6Params& p, hipStream_t s);
void launch_split6_inverse(const Split6Params& p, hipStream_t s);
// F(4x4,3x3) filter transform of one (output, input) channel pair in double: u[6 r + q] = (G g G^T)[r][q] (kernels_wino4.hip)
void conv_wino4_filter(const double g[3][3], double u[36]);

// The decoder's ConvTranspose2d(k2, s2) on a kernel of its own (kernels_deconv.hip): a wave owns 16 input pixels and
// all four taps (or the two taps of one dy), so every input row is read once (twice); output pixel (2y + dy, 2x + dx) receives tap
// q = 2 dy + dx.  The K loop walks a host-made list of 4-channel groups: groups whose weights are all zero are not in it, and channels
// of a listed group whose weights are zero are masked out of the input (whatever they hold) and out of the weights.
struct DeconvK2S2Params {
    static constexpr int MAX_GROUPS = 48;   // 192 live input channels
    const float* x;            // NHWC [B, H, W, in_ld], the first Cin channels used
    int B, H, W, Cin, in_ld;   // Cin, in_ld: multiples of 4
    const float* wpk;          // packed weights [>= 4 cw][Kpad], row q * cw + o, column = input channel (PackedConv::w of a 1x1 GEMM)
    int Kpad;
    const float* bias;         // [4 cw]
    float* out;                // NHWC [B, 2H, 2W, ld]: channels [coff, coff + cw) are written
    int ld, coff, cw;          // ld, coff: multiples of 4; cw: a multiple of 16
    // deconv_k2s2_prepare:
    int ngroups;               // listed groups, a multiple of 4 (padded with masked groups)
    unsigned jmasked;          // bit j: one of the groups 4j .. 4j + 3 has a masked channel
    unsigned short gch[MAX_GROUPS];   // first channel of group g
    unsigned char gmask[MAX_GROUPS];  // bit i: channel gch[g] + i is live
    int taps;                  // 4: one workgroup holds all the weights; 2: those of one dy (grid y = 2)
    unsigned fdw_mul, fdw_shift, fdh_mul, fdh_shift;   // m / W and (m / W) / H by multiply-shift
};
// Fills the group list from live[Cin] (live[c] != 0: some weight of input channel c is not zero; null: every channel is) and chooses
// the form; false: the kernel does not take these sizes (pointers are not looked at)
bool deconv_k2s2_prepare(DeconvK2S2Params& p, const unsigned char* live);
void launch_deconv_k2s2(const DeconvK2S2Params& p, hipStream_t s);

// the angle of the test loops (train_VIGOR.py:307-311) in the fp32 form the post-processing kernels write
__device__ __forceinline__ float pose_angle_deg(float cs, float sn) {
    float ang = acosf(fminf(fmaxf(cs, -1.f), 1.f)) * 57.29577951308232f;
    if (sn < 0.f) { ang = fmodf(-ang, 360.f); if (ang < 0.f) ang += 360.f; }
    return ang;
}

// The output side's geometry: the map side (CCVPE_OUT_HW) and the chunks a map is reduced in - TAIL_CHUNKS workgroups per sample take
// 4096 values each; the last arriver's first wave holds one chunk per lane
static constexpr int TAIL_HW = 512, TAIL_CHUNKS = 64;
static_assert(TAIL_HW * TAIL_HW == TAIL_CHUNKS * 4 * 4 * 256 && TAIL_CHUNKS == 64, "four float4 per thread per chunk, one lane of a wave per chunk");

struct SoftmaxParams {
    const float* logits;       // [B][n]
    int B, n;
    float* partial;            // [B][chunks][2]
    int chunks;
    float* out;                // [B][n]
    const float* prior;        // optional [B][n] log-prior: partials of fl32(logit + prior); launch_softmax_partial only
    long long prior_stride;    //   floats between two samples' maps: 0 (one shared map) or n
};
void launch_softmax(const SoftmaxParams& p, hipStream_t s);
void launch_softmax_partial(const SoftmaxParams& p, hipStream_t s);   // the first of launch_softmax's two launches alone (pose plans)

// Pose plans: argmax of the softmax WITHOUT the heatmap.  Grid (64 chunks, B): every workgroup re-derives the sample's (max, 1/sum) from
// the softmax partials as softmax_final_kernel does, recomputes the heatmap values of its chunk in registers with the expression that
// kernel stores, and keeps the first maximal index; the last arriver of a sample (ticket) writes index[b] and rows[b][0..1].
struct PoseArgmaxParams {
    const float* logits;       // [B][n]
    const float* partial;      // [B][chunks][2] of softmax_partial_kernel
    int B, n, chunks;          // chunks == 64
    float* pairs;              // [B][chunks][2] (max, index) hand-off
    unsigned* tickets;         // [B] counters, zero before and after every launch
    int* index;                // [B] argmax, always in [0, n)
    float* rows;               // [B][5]: columns 0 (index) and 1 (prob)
    float* stats;              // optional [B][2]: the sample's softmax (max, 1/sum), written by workgroup (0, b) (ccvpe_localize_region)
    const float* prior;        // optional log-prior as SoftmaxParams::prior (the partials must be of the same sums).  A sample whose
    long long prior_stride;    //   (max, 1/sum) is not finite gets index 0 and rows (-1, NaN)
    float* posterior;          // optional [B][n] (ccvpe_track_update*): the heatmap of l' the chunks recompute, stored as
                               //   float4; all zeros (and the row (-1, NaN)) for a sample whose (max, 1/sum) is not finite
    float* summary;            // optional [B][SUMMARY_COLS] (ccvpe_*_summary): moments, entropy and peak mass of that heatmap;
    double* summ_part;         //   with it [B][chunks][SUMMARY_PART] float64 hand-off of the chunks' sums and
    int summary_r;             //   the half side 0 .. SUMMARY_MAX_R of the window around the argmax
};
void launch_pose_argmax(const PoseArgmaxParams& p, hipStream_t s);

// Posterior summary: one row of SUMMARY_COLS floats per map h of 512 x 512 values, x = index % 512, y = index / 512 -
//   0 argmax (first maximal index)   1 h there   2 S0 = sum h   3 entropy -sum (h/S0) ln(h/S0) over h > 0, nats
//   4, 5 mean x, y   6, 7, 8 var_xx, cov_xy, var_yy about it                            (weights h / S0)
//   9 sum of h over the window |x - x*| <= r, |y - y*| <= r around the argmax, clipped to the grid, over S0
//   10, 11 mean x, y of the window   12, 13, 14 its var_xx, cov_xy, var_yy about that mean   (weights h / the window's sum)   15 its cells
// from float64 sums (h times a coordinate product below 2^18 is exact in float64).  pose_argmax_kernel computes it for the heatmap it
// recomputes; launch_belief_summary for a stored map: grid (64 chunks, B), one launch, the same accumulation and reduction code.
static constexpr int SUMMARY_COLS = 16, SUMMARY_PART = 8, SUMMARY_MAX_R = 32;
struct BeliefSummaryParams {
    const float* belief;       // [B][512*512], 4-byte aligned (16-byte aligned maps are read as float4)
    int B, r;
    float* pairs;              // [B][64][2] (max, index) hand-off
    double* summ_part;         // [B][64][SUMMARY_PART]
    unsigned* tickets;         // [B] counters, zero before and after every launch
    float* summary;            // [B][SUMMARY_COLS]; S0 == 0: (0, 0, 0, NaN ...)
};
void launch_belief_summary(const BeliefSummaryParams& p, hipStream_t s);
// rows[b][2..4] = (cos, sin, angle_deg) of ori [B][2][n] at index[b] (pose plans without the fused level 1)
void launch_pose_gather(const float* ori, const int* index, int B, int n, float* rows, hipStream_t s);

// Heading posterior (kernels_heading.hip): the posterior h of pose_argmax_kernel (the same recomputed bits) as a
// distribution over the orientation field (c, s) = ori [B][2][n].  A cell is valid when c and s are finite and not both zero; its angle is
// pose_angle_deg(c, s) in [0, 360), its bin (int)(angle * nbins / 360), a result >= nbins wrapping to bin - nbins.  Per query
//   hist[nbins]   sum of h over the valid cells of each bin (absolute mass), and heading[HEADING_COLS]:
//   0 M = sum of h over valid cells   1, 2 C = sum h c / M, S = sum h s / M   3 atan2(S, C) in degrees [0, 360), NaN when R == 0
//   4 R = sqrt(C^2 + S^2)   5 mode bin (first maximal hist value)   6 hist[mode] / M
//   7 .. 11 columns 0 .. 4 over the window |x - x*| <= r, |y - y*| <= r around the argmax index[b], clipped to the grid.
// A sample whose (max, 1/sum) is not finite: hist all zero, heading NaN with column 5 = -1.  One launch on a grid (64 chunks, B): the
// histogram in 2^-52 fixed point (64-bit integer adds: LDS per workgroup, agent scope per query - no order to depend on), M, sum h c
// and sum h s as float64 in the fixed order of the summary; the last arriver of a sample (ticket) totals, runs the window and writes.
static constexpr int HEADING_COLS = 12, HEADING_PART = 4, HEADING_MIN_BINS = 4, HEADING_MAX_BINS = 360, HEADING_MAX_R = 32;
struct HeadingParams {
    const float* logits;       // [B][512*512]
    const float* partial;      // [B][64][2] of softmax_partial_kernel (of logits + prior when there is one)
    const float* prior;        // optional log-prior as PoseArgmaxParams::prior
    long long prior_stride;
    const float* ori;          // [B][2][512*512]
    const int* index;          // [B] argmax of pose_argmax_kernel, an earlier launch (clamped to the map before it is used)
    int B, nbins, r;           // nbins HEADING_MIN_BINS .. HEADING_MAX_BINS, r 0 .. HEADING_MAX_R: checked by the entry points
    double* part;              // [B][64][HEADING_PART] float64 hand-off of the chunks' sums
    unsigned long long* bins;  // [B][HEADING_MAX_BINS] the queries' fixed-point histograms: zero before and after every launch, like ...
    unsigned* tickets;         // ... the [B] counters
    float* heading;            // [B][HEADING_COLS]
    float* hist;               // [B][nbins]
};
void launch_heading_reduce(const HeadingParams& p, hipStream_t s);

// Credible regions (kernels_credible.hip; the definition is pinned in include/ccvpe.h): a radix select on the keys of a
// 512 x 512 map - the stored one, or pose_argmax_kernel's recomputed bits from logits (+ prior) and the softmax partials.  Per pass a grid
// (64 chunks, B) with a last arriver per query; CRED_PASSES launches and, with a level map, one more.  Integer adds only.
static constexpr int CRED_MAX_LEVELS = 8, CRED_DIGITS = 256, CRED_PASSES = 4, CRED_SLICE = 256;
struct CredState {             // per query: what a pass's last arriver leaves for the next launch
    unsigned long long Q;                         // the map's total mass (pass 0)
    unsigned long long T[CRED_MAX_LEVELS];        // the levels' thresholds T(p) (pass 0)
    unsigned long long above[CRED_MAX_LEVELS];    // mass and ...
    unsigned cabove[CRED_MAX_LEVELS];             // ... count of the keys above the level's prefix
    unsigned prefix[CRED_MAX_LEVELS];             // the digits fixed so far, in place; after the last pass k*
    unsigned group[CRED_MAX_LEVELS];              // the first level with the same prefix: its histogram row serves this level too
    unsigned alive, pad;                          // Q > 0
};
static_assert(sizeof(CredState) % 8 == 0, "an array of states keeps its 64-bit fields aligned");
struct CredibleParams {
    const float* belief;       // [B][512*512] stored map, 4-byte aligned (16-byte aligned maps are read as float4), or null: recompute from
    const float* logits;       //   [B][512*512] logits,
    const float* partial;      //   [B][64][2] softmax partials (of logits + prior when there is one) and
    const float* prior;        //   the optional log-prior as PoseArgmaxParams::prior
    long long prior_stride;
    const int* probe;          // optional [B] cell per query; an index outside the map is never dereferenced
    int B, n_levels;           // n_levels 1 .. CRED_MAX_LEVELS
    float level[CRED_MAX_LEVELS];   // the levels, by value
    unsigned long long* hmass; // [min(B, CRED_SLICE)][8][256] the queries' histograms, ...
    unsigned* hcnt;            // ... their counts and ...
    unsigned long long* pacc;  // ... [..][2] the probe's sums: zero before and after every launch, like ...
    unsigned* tickets;         // ... the [B] counters
    CredState* state;          // [min(B, CRED_SLICE)]
    float* cred;               // [B][4 + 3 n_levels]
    unsigned char* level_map;  // optional [B][512*512]
};
size_t credible_zero_words(int B);    // 32-bit words of the zeroed region for B queries (8-byte aligned start) ...
size_t credible_state_words(int B);   // ... and of the states
void credible_scratch(CredibleParams& p, int B, void* zeroed, void* state);   // hmass, hcnt, pacc and state over those two regions
void launch_credible(const CredibleParams& p, hipStream_t s);   // CRED_PASSES launches (+ 1 with a level map) per CRED_SLICE queries

// Top-K peaks (ccvpe_postprocess_topk / ccvpe_localize_topk).  Grid (64 tiles of 64 x 64, B): peaks of the heatmap
// under a Chebyshev radius r (value descending, index ascending), the best k per tile handed to the sample's last arriver (ticket),
// which writes index[b][k] (-1: no peak) and rows[b][k][0..1] - the whole row (-1, 0, 0, 0, 0) for a slot without a peak.
static constexpr int TOPK_MAX_K = 64, TOPK_MAX_R = 32;
struct TopkParams {
    const float* heat;          // [B][n] stored heatmap, or null: recompute it from
    const float* logits;        //   [B][n] logits and
    const float* partial;       //   [B][64][2] softmax partials (softmax_final_kernel's statistics and expression)
    int B, k, r;                // k 1..64, r 0..32
    unsigned long long* keys;   // [B][64][k] hand-off
    unsigned* tickets;          // [B] counters, zero before and after every launch
    int* index;                 // [B][k]
    float* rows;                // [B][k][5]
    const float* prior;         // optional log-prior of the logits path (SoftmaxParams::prior): values __expf((l + prior) - m) * inv;
    long long prior_stride;     //   a sample whose (m, inv) is not finite has no peak
};
void launch_topk_peaks(const TopkParams& p, hipStream_t s);
// rows[b][k][2..4] = (cos, sin, angle_deg) of ori [B][2][n] at index[b][k] >= 0 (postprocess_topk; pose plans without the fused level 1)
void launch_topk_gather(const float* ori, const int* index, int B, int K, int n, float* rows, hipStream_t s);
// ccvpe_postprocess_topk scratch for B samples: [PP_MAX_BATCH ticket counters][B x 64 x 64 keys][B x 64 indices]
size_t topk_scratch_bytes(int B);

struct PreprocParams {
    const unsigned char* in;   // [B][H][W][3] uint8
    int B, H, W, crop_w;
    const int* shift;          // [B] roll in pixels (out[x] = in[(x - shift) mod W]) or null
    float mean[3], stdv[3];
    float* out;                // [B][3][H][crop_w] fp32
};
void launch_preprocess(const PreprocParams& p, hipStream_t s);
// resize (PIL bilinear, byte-exact) + ToTensor + Normalize + roll + crop (kernels_preproc.hip)
struct ResizeParams {
    const unsigned char* in;   // [B][IH][IW][3] uint8
    int B, IH, IW, OH, OW, crop_w;
    unsigned char* tmp;        // [B][IH][OW][3] uint8 scratch (the horizontally resampled image)
    const int* shift;          // [B] roll in output pixels or null
    float mean[3], stdv[3];
    float* out;                // [B][3][OH][crop_w] fp32
    // window mode (origin != null): `in` is ONE map [map_h][map_w][3]; sample b resizes the IH x IW window whose top-left corner
    // is (origin[2b], origin[2b+1]) = (x0, y0), pixels outside the map read as 0 (PIL.Image.crop).  The width pass always runs.
    const int* origin;
    int map_h, map_w;
};
int launch_resize(const ResizeParams& p, hipStream_t s);   // -1: down-scaling factor above 8

// chain of PIL affine transforms (NEAREST / BILINEAR) + crop + ToTensor + Normalize (kernels_warp.hip)
static constexpr int WARP_MAX_STAGES = 4;
static constexpr int WARP_MAX_BILINEAR = 2;
struct WarpParams {
    const unsigned char* in;   // [B][H][W][3] uint8; every stage maps an H x W canvas onto an H x W canvas
    const double* mat;         // [B][n][6] PIL affine data (output pixel -> input position), stage 0 reads `in`
    int B, H, W, n;
    unsigned bilinear;         // bit s set: stage s resamples BILINEAR, else NEAREST
    int top, left, out_h, out_w;   // crop window of the last stage's canvas
    float mean[3], stdv[3];
    float* out;                // [B][3][out_h][out_w] fp32
};
int launch_warp(const WarpParams& p, hipStream_t s);       // -1: stage pattern without a kernel

void launch_scatter_channels(const float* src, int C, long long P, Dst d0, Dst d1, int ndst, hipStream_t s);
// the same copy with a per-sample source: destination sample b reads sample tile[b] of a section laid out for n_tiles samples
// ([n_tiles][hw][C], the indexed cached forms).  The indices travel by value in the launch arguments, GATHER_MAX_SAMPLES per launch.
static constexpr int GATHER_MAX_SAMPLES = 16;
struct GatherParams {
    const float* src;   // section base: [n_tiles][hw][C] fp32
    Dst d0, d1;
    int ndst;
    int C, hw;          // channels (multiple of 4), pixels per sample
    int b0;             // destination sample of blockIdx.y == 0
    int tile[GATHER_MAX_SAMPLES];   // source sample of destination sample b0 + blockIdx.y
};
void launch_gather_channels(const float* src, int C, int hw, const int* tile, int B, Dst d0, Dst d1, int ndst, hipStream_t s);

// Cross-tile reduction of ccvpe_localize_region: one 64-lane workgroup per query.  The pair offsets of the queries
// travel by value in the launch arguments, REGION_MAX_QUERIES queries per launch.  offsets: HOST [G+1], every range non-empty.
static constexpr int REGION_MAX_QUERIES = 64;
struct RegionParams {
    const float* stats;       // [P][2] (max, 1/sum) of each pair (PoseArgmaxParams::stats)
    const float* pair_rows;   // [P][5] pose rows of each pair
    float* rows;              // [G][5]
    int* best_pair;           // [G]
    float* tile_prob;         // [P]
    int g0;                   // query of blockIdx.x == 0
    int off[REGION_MAX_QUERIES + 1];   // pair offsets of queries g0 .. g0 + gridDim.x
};
void launch_region_reduce(const float* stats, const float* pair_rows, const int* offsets, int G, float* rows, int* best_pair, float* tile_prob,
                          hipStream_t s);

// Motion update of a position belief (ccvpe_track_predict, DESIGN.md 4.11, kernels_track.hip): per query the belief [512][512], zero
// outside, moved by (dx, dy) with bilinear weights, blurred along x then y with the symmetric taps t[|i|], i = -radius..radius, and
// log_prior = logf(that + floor[b]).  One launch, grid (256 tiles of 32 x 32, B).
static constexpr int TRACK_MAX_R = 32;
struct TrackPredictParams {
    const float* belief;       // [B][512*512]
    const float* shift;        // [B][2] = (dx, dy) in output pixels
    const float* taps;         // [radius + 1] one-sided weights, one set (taps_stride 0) or one per query (taps_stride radius + 1)
    int taps_stride;
    int radius;                // 0 .. TRACK_MAX_R
    const float* floor;        // [B] >= 0, added before the logarithm
    float* log_prior;          // [B][512*512], not aliasing belief
    int B;
};
void launch_track_predict(const TrackPredictParams& p, hipStream_t s);

// The same step under an affine map per query (ccvpe_track_predict_affine, DESIGN.md 4.14, kernels_track_affine.hip): output pixel
// index (x, y) reads the belief at index position (m0 x + m1 y + m2, m3 x + m4 y + m5), float64, bilinear weights from fractions
// rounded once to float32, times (float)|m0 m4 - m1 m3|; then the blur, the floor and the logarithm of launch_track_predict.  One
// launch, grid (256 tiles of 32 x 32, B).
struct TrackPredictAffineParams {
    const float* belief;       // [B][512*512]
    const double* matrix;      // [B][6] output index -> source index position
    const float* taps;         // [radius + 1] one-sided weights, one set (taps_stride 0) or one per query (taps_stride radius + 1)
    int taps_stride;
    int radius;                // 0 .. TRACK_MAX_R
    const float* floor;        // [B] >= 0, added before the logarithm
    float* log_prior;          // [B][512*512], not aliasing belief
    int B;
};
void launch_track_predict_affine(const TrackPredictAffineParams& p, hipStream_t s);

// Backward pass over stored beliefs (ccvpe_track_smooth, DESIGN.md 4.20, kernels_track_smooth.hip): per query the smoothed map of frame
// t from its filter posterior `belief`, the smoothed map `next` of frame t + 1 and the arguments of the launch_track_predict call
// between the two.  Three launches - grid (256 tiles, B) twice, then (64 chunks, B) - that hand over through `work` alone.
struct TrackSmoothParams {
    const float* belief;       // [B][512*512]
    const float* next;         // [B][512*512]; may be `smoothed`
    const float* shift;        // [B][2] = (dx, dy) of the predict call
    const float* taps;         // as TrackPredictParams
    int taps_stride;
    int radius;                // 0 .. TRACK_MAX_R
    const float* floor;        // [B] >= 0
    float* smoothed;           // [B][512*512]
    float* stats;              // [B][4] = (index, prob, Z, G)
    float* work;               // track_smooth_work_bytes(B) bytes, written before it is read: any contents
    int B;
};
size_t track_smooth_work_bytes(int B);
void launch_track_smooth(const TrackSmoothParams& p, hipStream_t s);
void launch_track_smooth_scale(const TrackSmoothParams& p, hipStream_t s);   // its last launch alone (work, smoothed, stats, B are read)
void launch_track_smooth_ratio(const TrackSmoothParams& p, hipStream_t s);   // its first launch alone (smoothed and stats are not read)

// Link statistics of a smoothed stream (ccvpe_track_link, DESIGN.md 4.25, kernels_track_link.hip): per query the posterior mass of
// every integer displacement the predict call between frames t and t + 1 can move a cell by, and of a jump through its floor, from the
// filter posterior `belief` of frame t, the smoothed map `next` of frame t + 1 and that call's arguments.  Four launches -
// launch_track_smooth_ratio, grid (256 tiles, B), (ceil((2r + 2)^2 / 256), B), (B) - that hand over through `work` alone.
struct TrackLinkParams {
    const float* belief;       // [B][512*512]
    const float* next;         // [B][512*512]; may be `belief`
    const float* shift;        // [B][2] = (dx, dy) of the predict call
    const float* taps;         // as TrackPredictParams
    int taps_stride;
    int radius;                // 0 .. TRACK_MAX_R
    const float* floor;        // [B] >= 0
    float* moves;              // [B][2r + 2][2r + 2]: row ky, column kx is the displacement (ix + r + 1 - kx, iy + r + 1 - ky)
    float* stats;              // [B][4] = (Z, G, J, M)
    float* work;               // track_link_work_bytes(B, radius) bytes, written before it is read: any contents
    int B;
};
size_t track_link_work_bytes(int B, int radius);
void launch_track_link(const TrackLinkParams& p, hipStream_t s);

// The same backward step behind a launch_track_predict_affine call (ccvpe_track_smooth_affine, DESIGN.md 4.22,
// kernels_track_smooth_affine.hip): the adjoint of the bilinear gather through `matrix` as a gather over the candidate samples of every
// cell, in a fixed order.  Four launches - (256 tiles, B), the tiles of the grid extended by the radius, (256 tiles, B), then
// launch_track_smooth_scale - that hand over through `work`: TrackSmoothParams' layout per query, then the blurred ratio map h.
struct TrackSmoothAffineParams {
    const float* belief;       // [B][512*512]
    const float* next;         // [B][512*512]; may be `smoothed`
    const double* matrix;      // [B][6] of the predict call: output index -> source index position
    const float* taps;         // as TrackPredictParams
    int taps_stride;
    int radius;                // 0 .. TRACK_MAX_R
    const float* floor;        // [B] >= 0
    float* smoothed;           // [B][512*512]
    float* stats;              // [B][4] = (index, prob, Z, G)
    float* work;               // track_smooth_affine_work_bytes(B) bytes, written before it is read: any contents
    int B;
};
size_t track_smooth_affine_work_bytes(int B);
void launch_track_smooth_affine(const TrackSmoothAffineParams& p, hipStream_t s);

// MAP trajectory of a tracked stream (ccvpe_track_viterbi, DESIGN.md 4.23, kernels_track_viterbi.hip): per query the max-product score
// map of frame t from its filter posterior `belief`, the posterior `belief_prev` and the score map `score_prev` of frame t - 1 and the
// arguments of the launch_track_predict call between the two.  belief_prev, score_prev, prev_stats and shift all null: the first frame
// of a stream, score = belief.  Two launches - grid (256 tiles, B), then (64 chunks, B) - that hand over through `work` alone.
struct TrackViterbiParams {
    const float* belief;       // [B][512*512]
    const float* belief_prev;  // [B][512*512] or null
    const float* score_prev;   // [B][512*512] or null
    const float* prev_stats;   // [B][4], the stats of the call that made score_prev, or null
    const float* shift;        // [B][2] = (dx, dy) of the predict call, or null
    const float* taps;         // as TrackPredictParams
    int taps_stride;
    int radius;                // 0 .. TRACK_MAX_R
    const float* floor;        // [B] >= 0
    float* score;              // [B][512*512], aliasing no input map
    float* stats;              // [B][4] = (index, peak, exponent, restarted)
    float* work;               // track_viterbi_work_bytes(B) bytes, written before it is read: any contents
    int B;
};
size_t track_viterbi_work_bytes(int B);
void launch_track_viterbi(const TrackViterbiParams& p, hipStream_t s);

// One link of the backtrack (ccvpe_track_viterbi_back): per query the cell of frame t - 1 that the path's `cell` of frame t came from
// and the link's kind, from the score map of frame t - 1 and the arguments of the predict call between the two.  One launch, grid (B).
enum ViterbiLink { VITERBI_LINK_MOVE = 0, VITERBI_LINK_JUMP = 1, VITERBI_LINK_START = 2 };
struct TrackViterbiBackParams {
    const float* score_prev;   // [B][512*512]
    const float* prev_stats;   // [B][4]
    const int* cell;           // [B]; outside [0, 512*512): the backtrack starts here
    const float* shift;        // [B][2]
    const float* taps;         // as TrackPredictParams
    int taps_stride;
    int radius;
    const float* floor;        // [B]
    int* back;                 // [B][2] = (previous cell or -1, ViterbiLink)
    int B;
};
void launch_track_viterbi_back(const TrackViterbiBackParams& p, hipStream_t s);
void launch_track_viterbi_scale(const TrackViterbiParams& p, hipStream_t s);   // its last launch alone (work, score, stats, B, and for
                                                                               // `restarted` belief_prev, score_prev, prev_stats are read)

// The same two calls behind a launch_track_predict_affine call (ccvpe_track_viterbi_affine, ccvpe_track_viterbi_back_affine, DESIGN.md
// 4.24, kernels_track_viterbi_affine.hip): the move is read as a latent choice of the sample position the blur reads and of the one of
// its four bilinear taps that carried the mass, so a link's maximum is a four-tap max-gather through `matrix` followed by the max passes
// over the 2r + 1 symmetric taps.  Two launches - grid (256 tiles, B), then launch_track_viterbi_scale - through TrackViterbiParams'
// work; belief_prev null (with score_prev, prev_stats, matrix): launch_track_viterbi's first-frame form itself.
struct TrackViterbiAffineParams {
    const float* belief;       // [B][512*512]
    const float* belief_prev;  // [B][512*512] or null
    const float* score_prev;   // [B][512*512] or null
    const float* prev_stats;   // [B][4] or null
    const double* matrix;      // [B][6] of the predict call: output index -> source index position, or null
    const float* taps;         // as TrackPredictParams
    int taps_stride;
    int radius;                // 0 .. TRACK_MAX_R
    const float* floor;        // [B] >= 0
    float* score;              // [B][512*512], aliasing no input map
    float* stats;              // [B][4] = (index, peak, exponent, restarted)
    float* work;               // track_viterbi_work_bytes(B) bytes
    int B;
};
void launch_track_viterbi_affine(const TrackViterbiAffineParams& p, hipStream_t s);

struct TrackViterbiBackAffineParams {
    const float* score_prev;   // [B][512*512]
    const float* prev_stats;   // [B][4]
    const int* cell;           // [B]; outside [0, 512*512): the backtrack starts here
    const double* matrix;      // [B][6]
    const float* taps;         // as TrackPredictParams
    int taps_stride;
    int radius;
    const float* floor;        // [B]
    int* back;                 // [B][2] = (previous cell or -1, ViterbiLink)
    int B;
};
void launch_track_viterbi_back_affine(const TrackViterbiBackAffineParams& p, hipStream_t s);

// Heading prior (kernels_hprior.hip).  The combined prior map of a heading table T [nb + 1] (log-weights of the heading
// bins of DESIGN.md 4.13, entry nb for a cell without a heading) and an optional position prior P: per cell
// out = T[k] or fl32(P + T[k]), k = the cell's bin by heading_reduce_kernel's own expression, nb for an invalid cell.  One launch,
// grid (64 chunks, B); the result is the log_prior (stride 512 * 512) of any prior form.
struct HeadingPriorMapParams {
    const float* ori;          // [B][2][512*512]
    const float* prior;        // optional position log-prior as PoseArgmaxParams::prior
    long long prior_stride;
    const float* table;        // [nb + 1] one table (table_stride 0) or one per query (table_stride nb + 1)
    int table_stride;
    int nb;                    // HEADING_MIN_BINS .. HEADING_MAX_BINS: checked by the entry points
    float* out;                // [B][512*512], not aliasing ori or prior
    int B;
};
void launch_heading_prior_map(const HeadingPriorMapParams& p, hipStream_t s);

// Motion update of a heading belief (ccvpe_heading_predict): per query hist [nb] turned by turn_deg (linear weights between the two
// source bins, on the circle), blurred with the symmetric taps t[|j|], j = -radius..radius, and out[b] = logf(that + floor); out[nb],
// the weight of a cell without a heading, is what the average bin gets.  One launch, grid (B).
struct HeadingPredictParams {
    const float* hist;         // [B][nb], non-negative
    const float* turn_deg;     // [B]
    const float* taps;         // [radius + 1] one-sided weights, one set (taps_stride 0) or one per query (taps_stride radius + 1)
    int taps_stride;
    int radius;                // 0 .. TRACK_MAX_R, 2 radius + 1 <= nb
    const float* floor;        // [B] >= 0, added before the logarithm
    float* out;                // [B][nb + 1], not aliasing hist
    int B, nb;
};
void launch_heading_predict(const HeadingPredictParams& p, hipStream_t s);

// Joint position-heading filter (ccvpe_track_joint_*, DESIGN.md 4.26, kernels_track_joint.hip): the state is one [512][512] map per
// heading bin of DESIGN.md 4.13, joint [B][nb][512*512], linear and non-negative.  Predict: launch_track_predict's c of every slice
// under its own shift into `work` - grid (256 tiles, B * nb) - then per cell the turn and the blur on the circle of bins, plus the
// floor - grid (1024 groups of 256 cells, B).  Two launches.
static constexpr int JOINT_MIN_BINS = HEADING_MIN_BINS, JOINT_MAX_BINS = 72, JOINT_MAX_SLICES = 32768, JOINT_COLS = 5;
struct TrackJointPredictParams {
    const float* joint;        // [B][nb][512*512]
    const float* shift;        // [B][nb][2] = (dx, dy) in output pixels of every SOURCE bin
    const float* taps;         // as TrackPredictParams
    int taps_stride;
    int radius;                // 0 .. TRACK_MAX_R
    const float* turn_deg;     // [B]
    const float* htaps;        // [hradius + 1] one-sided weights on the circle, one set (htaps_stride 0) or one per query (hradius + 1)
    int htaps_stride;
    int hradius;               // 0 .. TRACK_MAX_R, 2 hradius + 1 <= nb
    const float* floor;        // [B] >= 0
    float* work;               // track_joint_work_bytes(B, nb) bytes, written before it is read: any contents
    float* prior;              // [B][nb][512*512], not aliasing joint or work
    int B, nb;
};
size_t track_joint_work_bytes(int B, int nb);
void launch_track_joint_predict(const TrackJointPredictParams& p, hipStream_t s);

// Update: U(k, i) = (__expf(l_i - m) * E(k | i)) * prior(k, i), Z its float64 sum, J' = U * (float)(1 / Z) with the marginal over the
// bins, the mass per bin and a row per query.  Four launches, grid (64 chunks, B) three times and (B): softmax_partial_kernel for m;
// the sum (the prior read once, nothing of the joint written); the store (U recomputed, the prior read again, J' written once);
// the finish.  The hand-offs are launch boundaries; every sum has one order.
struct TrackJointUpdateParams {
    const float* logits;       // [B][512*512]
    const float* ori;          // [B][2][512*512]
    const float* prior;        // [B][nb][512*512] or null (1 everywhere); may be joint_out
    const float* emission;     // [nb + 1] non-negative weights, one table (emission_stride 0) or one per query (nb + 1)
    int emission_stride;
    float* rows;               // [B][JOINT_COLS]
    float* joint_out;          // [B][nb][512*512]
    float* marginal;           // [B][512*512]
    float* hist;               // [B][nb]
    float* partial;            // scratch [B][64][2] softmax partials
    float* pairs;              // scratch [B][64][2] (max, first index) of the marginal per chunk
    double* zpart;             // scratch [B][64] the chunks' sums of U
    double* hpart;             // scratch [B][JOINT_MAX_BINS][64] the chunks' sums of J' per bin
    int B, nb;
};
size_t track_joint_scratch_bytes(int B);   // partial, pairs, zpart, hpart of B queries, in TrackJointUpdateParams' order from the back
void track_joint_scratch(void* scratch, int cap, TrackJointUpdateParams& p);   // ... carved out of a buffer of `cap` queries
void launch_track_joint_update(const TrackJointUpdateParams& p, hipStream_t s);

// The first launch of the predict alone: the backward step (kernels_track_joint_smooth.hip) starts with it, so its A is the predict's
// bits.  p.prior is not used.
void launch_track_joint_xy(const TrackJointPredictParams& p, hipStream_t s);

// The second launch of the predict alone, on a `work` that already holds A: the affine predict (kernels_track_joint_affine.hip) ends
// with it, so its heading mix is the predict's bit for bit.  p.joint, p.shift, p.taps, p.taps_stride and p.radius are not used.
void launch_track_joint_mix(const TrackJointPredictParams& p, hipStream_t s);

// The predict under an affine map per SOURCE heading bin (ccvpe_track_joint_predict_affine, DESIGN.md 4.30,
// kernels_track_joint_affine.hip): launch_track_predict_affine's c of every slice under its own matrix into `work` - grid (256 tiles,
// B * nb) - then launch_track_joint_mix.  Two launches.
struct TrackJointPredictAffineParams {
    const float* joint;        // [B][nb][512*512]
    const double* matrix;      // [B][nb][6] output index -> source index position of every SOURCE bin
    const float* taps;         // as TrackPredictParams
    int taps_stride;
    int radius;                // 0 .. TRACK_MAX_R
    const float* turn_deg;     // as TrackJointPredictParams, from here ...
    const float* htaps;
    int htaps_stride;
    int hradius;
    const float* floor;
    float* work;
    float* prior;              // ... to here
    int B, nb;
};
void launch_track_joint_predict_affine(const TrackJointPredictAffineParams& p, hipStream_t s);

// The backward step of the joint filter (ccvpe_track_joint_smooth, DESIGN.md 4.27, kernels_track_joint_smooth.hip): the smoothed joint
// of frame t from the stored filter joint J, the smoothed joint s' of frame t + 1 and the arguments of the predict that carried J
// into frame t + 1.  Five launches - launch_track_joint_xy, the ratio (1024 groups, B), the weight (256 tiles, B * nb), the scale
// (64 chunks, B), the finish (B) - that hand over through `work`: one joint-sized buffer (A, then h over it), then the partial sums.
struct TrackJointSmoothParams {
    const float* joint;        // [B][nb][512*512] J
    const float* next;         // [B][nb][512*512] s'; may be smoothed
    const float* shift;        // as TrackJointPredictParams, from here ...
    const float* taps;
    int taps_stride;
    int radius;
    const float* turn_deg;
    const float* htaps;
    int htaps_stride;
    int hradius;
    const float* floor;        // ... to here
    float* work;               // track_joint_smooth_work_bytes(B, nb) bytes, written before it is read: any contents
    float* smoothed;           // [B][nb][512*512]
    float* marginal;           // [B][512*512]
    float* hist;               // [B][nb]
    float* stats;              // [B][JOINT_SMOOTH_COLS] = (index, prob, bin, Z, G)
    int B, nb;
};
static constexpr int JOINT_SMOOTH_COLS = 5;
size_t track_joint_smooth_work_bytes(int B, int nb);
void launch_track_joint_smooth(const TrackJointSmoothParams& p, hipStream_t s);

// MAP trajectory of a joint stream (ccvpe_track_joint_viterbi, DESIGN.md 4.29, kernels_track_joint_viterbi.hip): per query the
// max-product score joint of frame t from its filter joint J, the joint J- and the score joint v- of frame t - 1 and the arguments of
// the launch_track_joint_predict call between the two.  joint_prev, score_prev, prev_stats and shift all null: the first frame of a
// stream, score = J.  Four launches - launch_track_joint_xy on J-, the win (256 tiles, B * nb), the mix (1024 groups, B), the scale
// (16 parts, B * nb) - that hand over through `work`: A, win, then the groups' pairs; the first frame runs the last two alone.
static constexpr int JOINT_VITERBI_COLS = 5;
struct TrackJointViterbiParams {
    const float* joint;        // [B][nb][512*512] J
    const float* joint_prev;   // [B][nb][512*512] J- or null
    const float* score_prev;   // [B][nb][512*512] v- or null
    const float* prev_stats;   // [B][JOINT_VITERBI_COLS], the stats of the call that made score_prev, or null
    const float* shift;        // as TrackJointPredictParams, from here ... (null in the first-frame form)
    const float* taps;
    int taps_stride;
    int radius;
    const float* turn_deg;
    const float* htaps;
    int htaps_stride;
    int hradius;
    const float* floor;        // ... to here
    float* work;               // track_joint_viterbi_work_bytes(B, nb) bytes, written before it is read: any contents
    float* score;              // [B][nb][512*512], aliasing no input
    float* stats;              // [B][JOINT_VITERBI_COLS] = (index, bin, peak, exponent, restarted)
    int B, nb;
};
size_t track_joint_viterbi_work_bytes(int B, int nb);
void launch_track_joint_viterbi(const TrackJointViterbiParams& p, hipStream_t s);

// One link of its backtrack (ccvpe_track_joint_viterbi_back): per query the (cell, bin) of frame t - 1 that the path's (cell, bin) of
// frame t came from and the link's kind.  One launch, grid (B).
struct TrackJointViterbiBackParams {
    const float* score_prev;   // [B][nb][512*512]
    const float* prev_stats;   // [B][JOINT_VITERBI_COLS]
    const int* cell;           // [B]; outside [0, 512*512): the backtrack starts here
    const int* bin;            // [B]; outside [0, nb): likewise
    const float* shift;        // as TrackJointPredictParams, from here ...
    const float* taps;
    int taps_stride;
    int radius;
    const float* turn_deg;
    const float* htaps;
    int htaps_stride;
    int hradius;
    const float* floor;        // ... to here
    int* back;                 // [B][3] = (previous cell or -1, previous bin or -1, ViterbiLink)
    int B, nb;
};
void launch_track_joint_viterbi_back(const TrackJointViterbiBackParams& p, hipStream_t s);

struct PoseOut { int32_t index; float prob, cos_v, sin_v, angle_deg; };
static constexpr int PP_MAX_BATCH = 4096;           // samples per launch_postprocess call
size_t postprocess_scratch_bytes(int B);            // partial (max, index) pairs + one ticket counter per sample (the counters zero before the first launch)
void launch_postprocess(const float* heat, const float* ori, int B, int n, PoseOut* out, float* rows, void* scratch, hipStream_t s);   // rows != null: [B][5] floats instead of `out`

struct MetricsOut { double pixel_distance, meter_distance, prob_at_gt, angle_pred_deg, angle_gt_deg, orientation_error_deg, longitudinal_m, lateral_m; };
void launch_metrics(const PoseOut* pose, const float* heat, int B, int W, int n, const int* gt_index, const float* gt_cos_sin,
                    const double* meter_per_pixel, const double* heading_deg, MetricsOut* out, hipStream_t s);

// several device-to-device copies in ONE launch (float counts, all pointers 16-byte aligned, counts multiples of 4): the staging
// copies around a hipGraph replay - 11 runtime copy launches of ~5 us each per batch-1 frame otherwise
struct MultiCopy { const float* src[12]; float* dst[12]; unsigned long long n[12]; int count; };
void launch_multi_copy(const MultiCopy& mc, hipStream_t s);
void launch_fill_random(float* p, size_t n, uint32_t seed, hipStream_t s);   // ~N(0,1) floats (autotune operands)
void launch_nhwc_to_nchw(const float* in, int in_ld, int coff, int C, int B, int HW, float* out, hipStream_t s);

}  // namespace ccvpe
