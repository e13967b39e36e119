// Internal declarations shared by the translation units of the host side of libccvpe_hip.so:
//   ccvpe_weights.hip  state_dict ingestion (BN folding, weight packing, Winograd transforms), packed-weight cache
//   ccvpe_plan.hip     the execution plan: CVM_*.forward restated as a static launch list over NHWC tensors
//   ccvpe_tune.hip     per-layer tile selection by measurement, the persistent tuning table, plan lookup
//   ccvpe_api.hip      the C ABI (include/ccvpe.h): handle lifetime, forward orchestration, diagnostics
#pragma once
#include "../../include/ccvpe.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <optional>
#include <set>
#include <string>
#include <type_traits>
#include <vector>

using namespace ccvpe;

// ------------------------------------------------------------------------------------------------
// errors (defined in ccvpe_api.hip)
// ------------------------------------------------------------------------------------------------
std::string& ccvpe_err();                       // thread-local message behind ccvpe_last_error()
int ccvpe_fail(int code, const char* fmt, ...);
#define HIPCHK(expr)                                                                           \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) return ccvpe_fail(CCVPE_EHIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// ------------------------------------------------------------------------------------------------
// static description of the network (mirrors ccvpe_amd/spec.py; reference lines cited there)
// ------------------------------------------------------------------------------------------------
struct BlockSpec { int e, k, s, cin, cout; };
static const BlockSpec B0[16] = {
    {1, 3, 1, 32, 16}, {6, 3, 2, 16, 24}, {6, 3, 1, 24, 24}, {6, 5, 2, 24, 40}, {6, 5, 1, 40, 40},
    {6, 3, 2, 40, 80}, {6, 3, 1, 80, 80}, {6, 3, 1, 80, 80}, {6, 5, 1, 80, 112}, {6, 5, 1, 112, 112},
    {6, 5, 1, 112, 112}, {6, 5, 2, 112, 192}, {6, 5, 1, 192, 192}, {6, 5, 1, 192, 192}, {6, 5, 1, 192, 192},
    {6, 3, 1, 192, 320},
};
static const int TAP_BLOCK[5] = {15, 10, 4, 2, 0};   // skip of decoder level 6..2 (models.py:465-469)
static const float BN_EPS = 1e-3f;                   // utils.py:666

struct DecLevel { int din, dout, skip, mid, out; };
struct VariantSpec {
    int feat_h;
    int head_ch[6];
    int sat_desc;
    int match_ch[6];
    int step[6];
    int n_rolls;
    int centre;
    DecLevel loc[6], ori[6];
};
static const DecLevel VIGOR_LOC[6] = {{1281, 1024, 320, 640, 640}, {641, 320, 112, 320, 320}, {321, 160, 40, 160, 160},
                                      {161, 80, 24, 80, 80},       {81, 40, 16, 40, 40},      {41, 16, 0, 16, 1}};
static const DecLevel VIGOR_ORI[6] = {{1300, 1024, 320, 640, 640}, {640, 256, 112, 256, 256}, {256, 128, 40, 128, 128},
                                      {128, 64, 24, 64, 64},       {64, 32, 16, 32, 32},      {32, 16, 0, 16, 2}};
static const DecLevel KITTI_LOC[6] = {{2049, 1024, 320, 512, 512}, {513, 256, 112, 256, 256}, {257, 128, 40, 128, 128},
                                      {129, 64, 24, 128, 128},     {129, 32, 16, 32, 32},     {33, 16, 0, 16, 1}};
static const DecLevel KITTI_ORI[6] = {{2064, 1024, 320, 512, 512}, {512, 256, 112, 256, 256}, {256, 128, 40, 128, 128},
                                      {128, 64, 24, 64, 64},       {64, 32, 16, 32, 32},      {32, 16, 0, 16, 2}};

static VariantSpec make_variant(int v) {
    VariantSpec s{};
    auto cp = [](DecLevel* d, const DecLevel* src) { for (int i = 0; i < 6; ++i) d[i] = src[i]; };
    if (v == CCVPE_VARIANT_KITTI) {
        s.feat_h = 8;
        int hc[6] = {16, 8, 4, 2, 1, 1}, mc[6] = {2048, 512, 256, 128, 128, 32}, st[6] = {128, 64, 32, 16, 8, 8};
        for (int i = 0; i < 6; ++i) { s.head_ch[i] = hc[i]; s.match_ch[i] = mc[i]; s.step[i] = st[i]; }
        s.sat_desc = 2048; s.n_rolls = 16; s.centre = 0;
        cp(s.loc, KITTI_LOC); cp(s.ori, KITTI_ORI);
    } else {
        int mc[6] = {1280, 640, 320, 160, 80, 40}, st[6] = {64, 32, 16, 8, 4, 2};
        int hv[6] = {64, 32, 16, 8, 4, 2}, ho[6] = {32, 16, 8, 4, 2, 1};
        for (int i = 0; i < 6; ++i) {
            s.match_ch[i] = mc[i]; s.step[i] = st[i];
            s.head_ch[i] = (v == CCVPE_VARIANT_OXFORD) ? ho[i] : hv[i];
        }
        s.feat_h = (v == CCVPE_VARIANT_OXFORD) ? 4 : 10;
        s.sat_desc = 1280; s.n_rolls = 20; s.centre = (v == CCVPE_VARIANT_OXFORD);
        cp(s.loc, VIGOR_LOC); cp(s.ori, VIGOR_ORI);
    }
    return s;
}

static void static_pad(int k, int s, int& lo, int& hi) {   // utils.py:261-277 with the nominal-224 walk
    if (s == 1) { lo = hi = (k - 1) / 2; return; }
    int total = k - 2;
    lo = total / 2; hi = total - lo;
}
static int conv_out(int n, int k, int s) {
    int lo, hi; static_pad(k, s, lo, hi);
    return (n + lo + hi - k) / s + 1;
}
static int se_squeeze(int cin) { return std::max(1, (int)(cin * 0.25)); }   // model.py:79
static int round_up(int a, int b) { return (a + b - 1) / b * b; }
// Width the transposed conv of a decoder level occupies in its concat buffer (round 4).  Channel-slice writes into the buffers are slow
// when a pixel's piece is not a whole number of 64-byte lines (tools/ubench_strided_write.py: 40 of 56 channels 3.4 TB/s against 5.3
// dense): the localisation decoder's level 2 (40 + 16 channels) is therefore laid out as [40 | 8 zero | 16] - 64 channels, pieces of
// 192 and 64 bytes; the transposed conv has eight zero output columns (it writes the zeros), conv2.0 eight zero input columns.
// pad = false (CCVPE_PAD_CONCAT=0): the reference's widths.  Every other level of every variant already ends on a line.
static int deconv_width(const DecLevel& l, bool pad) {
    return (pad && l.skip > 0 && (l.dout * 4) % 64 != 0) ? round_up(l.dout, 16) : l.dout;
}

// ------------------------------------------------------------------------------------------------
// environment switches: read once per handle by read_switches() (ccvpe_api.hip) at ccvpe_create.  Defaults are the
// library's behaviour with nothing set; the comment of each field names its variable and the setting that changes it.
// ------------------------------------------------------------------------------------------------
struct Switches {
    // handle
    bool autotune = true;                 // CCVPE_AUTOTUNE=0: plans the tuning table does not cover run the shape heuristic's tiles
    int fuse_mbconv = 1;                  // CCVPE_FUSE_MBCONV: 0 never, 1 where measured profitable (3x3 blocks), 2 every supported block
    bool fuse_level1 = true;              // CCVPE_FUSE_L1=0 falls back to deconv / conv / tail launches
    int l1_tile = 1;                      // CCVPE_L1_TILE=0: the fused last level on 16 x 16 output tiles (1: 32 wide x 16 high)
    // CCVPE_COMPOSE_L6: unset = fp32 plans of at least LEVEL6_AUTO_MIN_BATCH samples run decoder level 6 composed, 0 = never
    // (deconv, conv_a and its reduction as before), 1 = every fp32 plan, as F(4x4,2x2); 2 = every fp32 plan, as F(2x2,2x2) (for A/B runs)
    std::optional<int> compose_l6;
    // CCVPE_SPLIT_L6: conv6.2 and the skip half of conv6.0 in split Winograd form on the grouped GEMM (transform, GEMM,
    // inverse transform) where the composed level 6 runs.  unset = plans of at least LEVEL6_SPLIT_MIN_BATCH samples, 0 = never (the tiled
    // launches and their reductions), 1 = every plan that runs the composed level 6; 2 / 3 = as 1, conv6.2 only / the skip half only
    std::optional<int> split_l6;
    // CCVPE_DECONV_K2S2: the decoder's transposed convs on deconv_k2s2_kernel (kernels_deconv.hip).  unset = fp32 plans of
    // at least DECONV_K2S2_MIN_BATCH samples on level 2, DECONV_K2S2_MIN_BATCH_L3 on level 3; 0 = never (the tiled launches); 1 = every fp32 plan, on
    // every level whose shapes the kernel takes
    std::optional<int> deconv_k2s2;
    // CCVPE_WINOGRAD=0 keeps the decoder 3x3 layers on the implicit GEMM.  The Winograd kernels serve fp32 plans only: bf16x3 plans keep the
    // decoder tensors as split bf16 planes, which only the bf16x3 tiles read
    bool wino = true;
    int graph_mode = 0;                   // 1: plans replay a captured hipGraph (CCVPE_GRAPH=1; opt-in since round 4, see build_plan), 0 eager launches
    bool two_streams = true;              // CCVPE_STREAMS=1 issues everything on the caller's stream
    std::optional<int> precision;         // CCVPE_PRECISION: 1 for "bf16x3", 0 for anything else; unset: the config's
    // plan
    bool stem_dw = true;                  // CCVPE_STEM_DW=0: stem and block 0's depthwise conv as two launches
    std::optional<int> front_spread;      // CCVPE_FRONT_SPREAD: work items a fused MBConv front may spread to (unset: by encoder)
    bool mbconv_image = true;             // CCVPE_MBCONV_IMAGE=0: no image-resident MBConv front
    bool se_ticket = true;                // CCVPE_SE_TICKET=0: squeeze-excite as launches of its own
    bool se_prologue = false;             // CCVPE_SE_PROLOGUE=1: squeeze-excite in the latency-form project GEMM's prologue
    bool split_planes = true;             // CCVPE_NO_SPLIT_PLANES: bf16x3 plans keep every tensor fp32
    bool match_prep_early = true;         // CCVPE_MATCH_PREP_EARLY=0: each matching level prepares inside its own launch
    bool match_wide = true;               // CCVPE_MATCH_WIDE=0: the batch-32 form of the matching kernels at every batch
    bool issue_interleaved = true;        // CCVPE_ISSUE_ORDER=0: two-stream plans are issued in plan order
    bool log_schedule = false;            // CCVPE_LOG_SCHEDULE: print the two-stream schedule to stderr
    bool no_reuse = false;                // CCVPE_NO_REUSE: every tensor keeps its memory
    // tuner candidate filters (tests and diagnostics)
    bool tune_prefer_pw = false;          // CCVPE_TUNE_PREFER_PW: pointwise tiles wherever they apply
    bool tune_prefer_proj = false;        // CCVPE_TUNE_PREFER_PROJ: the deep-K project GEMM wherever it applies ...
    bool tune_prefer_lat = false;         // ... =lat: its latency form only
    std::optional<int> tune_splitk;       // CCVPE_TUNE_SPLITK=0: no split-K candidates
    bool tune_no_bf16x3 = false;          // CCVPE_TUNE_NO_BF16X3
    bool no_pw = false;                   // CCVPE_NO_PW: neither the pointwise nor the deep-K project tiles
    bool tune_ignore_table = false;       // CCVPE_TUNE_IGNORE_TABLE: measure every plan
    bool tune_lat_rows = false;           // CCVPE_TUNE_LAT_ROWS: also time the multi-row latency tiles
    bool tune_lat_split = false;          // CCVPE_TUNE_LAT_SPLIT: also time split-K latency tiles
    bool tune_no_fused_split = false;     // CCVPE_TUNE_NO_FUSED_SPLIT: no self-reducing split-K candidates
    std::string tune_verbose;             // CCVPE_TUNE_VERBOSE=<name part>: print every candidate of the matching launches
    // packer (part of the packed-weight cache key: pack_group())
    bool no_proj = false;                 // CCVPE_NO_PROJ
    int wino4_min_n = 40;                 // CCVPE_WINO4_MIN_N
    bool no_wino4 = false;                // CCVPE_NO_WINO4
    bool no_wino4x = false;               // CCVPE_NO_WINO4X
    bool pad_concat = true;               // CCVPE_PAD_CONCAT=0 (deconv_width)
    // diagnostics: CCVPE_DIAG_SYNC_BEFORE=<name part> drains the device before matching launches; CCVPE_DIAG_SNAP=<launch name> copies
    // that launch's tensors aside (stream ordered) right before and right after it
    std::string diag_sync, diag_snap;

    // a candidate filter is set: plans are measured under it, table or not, and their choices are not recorded (ccvpe_tune.hip)
    bool tune_filtered() const {
        return tune_prefer_pw || tune_prefer_proj || tune_splitk || tune_no_bf16x3 || no_pw || tune_ignore_table || tune_lat_rows || tune_lat_split ||
               tune_no_fused_split;
    }
    // the packer switches that differ from their defaults, as "NAME=value;" in a fixed order ("" when none does)
    std::string pack_group() const {
        std::string s;
        if (no_proj) s += "CCVPE_NO_PROJ=1;";
        if (wino4_min_n != 40) s += "CCVPE_WINO4_MIN_N=" + std::to_string(wino4_min_n) + ";";
        if (no_wino4) s += "CCVPE_NO_WINO4=1;";
        if (no_wino4x) s += "CCVPE_NO_WINO4X=1;";
        if (!pad_concat) s += "CCVPE_PAD_CONCAT=0;";
        return s;
    }
};
Switches read_switches();

// ------------------------------------------------------------------------------------------------
// weights
// ------------------------------------------------------------------------------------------------
struct PackedConv {
    float* w = nullptr;
    unsigned short *w_hi = nullptr, *w_lo = nullptr;   // bf16x3 planes (precision mode 1 only)
    float* bias = nullptr;
    int N = 0, Kpad = 0, nchunks = 0, cinp = 0, KH = 1, KW = 1;
    float* wino = nullptr;        // Winograd-domain weights of a 3x3 layer (kernels_wino.hip), fp32 mode only
    int wino_n16 = 0;
    size_t wino_bytes = 0;
    float* wino4 = nullptr;       // F(4x4,3x3) weights (kernels_wino4.hip): wide layers on maps up to 128 x 128 only
    size_t wino4_bytes = 0;
    float* wino4x = nullptr;      // xi-split F(4x4,3x3) weights (kernels_wino4x.hip): layers of 24 .. 128 output channels
    size_t wino4x_bytes = 0;
    int wino4x_cfg = -1;
    float* proj = nullptr;        // fragment-order copy of a gated deep-K 1x1 layer for kernels_proj.hip
    size_t proj_bytes = 0;
};
struct BlockW {
    PackedConv expand, project;
    float* exp_lin = nullptr;     // [mid][cinp16] expand weights for the fused expand+depthwise kernel
    int exp_cinp = 0;
    float *dw_w = nullptr, *dw_b = nullptr, *se_w1 = nullptr, *se_b1 = nullptr, *se_w2 = nullptr, *se_b2 = nullptr;
    int sq = 0;
};
struct EncoderW {
    float *stem_w = nullptr, *stem_b = nullptr;
    BlockW blk[16];
    PackedConv head;
};
struct DecoderW {
    PackedConv deconv[6], conva[6], convb[5];
    float* tail_w = nullptr;
    float* l1_wt = nullptr;       // the same weights as [9][cout][16] for the fused level-1 kernel (channel pairs contiguous)
    float tail_b[2] = {0.f, 0.f};
    // fused last level (kernels_level1.hip)
    float *l1_wc = nullptr, *l1_ws = nullptr, *l1_bc = nullptr;   // composed deconv + conv_a weights, score k-step, bias table (Level1Params)
    int l1_cx = 0, l1_cxp = 0, l1_c0 = 0, l1_ng = 0, l1_score = 0;
};
// Composed level 6 (kernels_level6.hip): derived from the packed weights of deconv[0] and conva[0] by ensure_level6, on the first plan
// that runs the composed path - never part of a packed-weight file (~0.35 GB per decoder)
struct Level6W {
    float* wc = nullptr;          // [4 P][Npad][Kc]
    float* bc = nullptr;          // [9][N]
    PackedConv skip;              // conv6.0's skip half (columns 1024 .. 1344) as a 3x3 convolution of its own, zero bias
    int K = 0, Kc = 0, N = 0, Npad = 0;
    // split form (Split6Params; ensure_level6_split): G g G^T of conv6.2 and of the skip half, [36][Npad][Kc] each, rounded once
    float* wb = nullptr;
    float* ws = nullptr;
};
static constexpr int LEVEL6_AUTO_MIN_BATCH = 8;   // the smallest batch at which the composed path measured faster (8, 16, 32 tried)
static constexpr int LEVEL6_SPLIT_MIN_BATCH = 8;  // ... and the split form of conv6.2 / the skip half (8, 16, 32 tried)
enum { SPLIT6_CONV_B = 1, SPLIT6_SKIP = 2 };      // Plan::l6_split
// deconv_k2s2_kernel under the automatic rule (profiles/deconv_k2s2_trace_b32_fp32.md): the smallest batch at which it
// measured faster than the tiled launches (8, 16, 32 tried) - level 2 from 8 samples, level 3 (a tie at 8) from 16; level 4 and up are
// wider than the kernel's slices
static constexpr int DECONV_K2S2_MIN_BATCH = 8;
static constexpr int DECONV_K2S2_MIN_BATCH_L3 = 16;
struct ccvpe_handle_s;
struct DecoderW;
// sizes of a decoder's composed level 6 from its packed descriptors (no device work); != 0: these weights cannot be composed
int level6_shape(const ccvpe_handle_s* h, const DecoderW& d, const struct DecLevel& l, int& K, int& Kc, int& N, int& Npad);
int ensure_level6(ccvpe_handle_s* h, int wm);   // 0, or an error code; wm = 4 or 2
int ensure_level6_split(ccvpe_handle_s* h);     // after ensure_level6: the split-form weights of both decoders; 0, or an error code
void release_level6(ccvpe_handle_s* h);
// the fused level's weights from the reference's layouts (ccvpe_weights.hip; the plan and ccvpe_op_level1 share them)
int compose_level1(ccvpe_handle_s* h, DecoderW& d, const std::vector<float>& w, const std::vector<float>& b, const std::vector<float>& wa,
                   const std::vector<float>& ba, int cin, int nscore);
int pack_level1_tail(ccvpe_handle_s* h, DecoderW& d, const std::vector<float>& w2, const std::vector<float>& b2, int cout);

struct Tensor {
    int id = -1; int B = 0, H = 0, W = 0, C = 0;
    bool split = false;   // bf16x3 mode: stored as two bf16 planes (hi | lo) instead of fp32
    long long numel() const { return (long long)B * H * W * C; }
};

// ------------------------------------------------------------------------------------------------
// The pose tail (softmax.partial -> pose.argmax or topk.peaks -> gather -> pose.heading): what a call asks of it, where its working
// memory is, and the four launches.  One definition for the plans (build_plan) and for the logits forms on the prior scratch
// (ccvpe_api.hip); every field is checked by the entry point that sets it.
// ------------------------------------------------------------------------------------------------
struct TailCall {
    float* rows = nullptr;             // [batch][5] result rows; top-K: [batch][topk_k][5]
    int topk_k = 0, topk_r = 0;        // topk_k > 0: the top-K tail (ccvpe_localize_topk*), hypotheses per query 1..64 and suppression radius 0..32
    const float* log_prior = nullptr;  // optional log-prior ...
    long long prior_stride = 0;        // ... and the floats between two queries' maps (0: one map for all)
    float* stats = nullptr;            // optional [batch][2] softmax (max, 1/sum) of each query (ccvpe_localize_region)
    float* posterior = nullptr;        // optional posterior maps [batch][512*512] (ccvpe_track_update*)
    float* summary = nullptr;          // optional [batch][16] summary rows (ccvpe_*_summary); selects the summary plans ...
    int summary_r = 0;                 // ... and their window radius 0..32
    float* heading = nullptr;          // optional [batch][12] heading rows (ccvpe_*_heading) and
    float* hist = nullptr;             //   [batch][heading_bins] histograms; select the heading plans ...
    int heading_bins = 0, heading_r = 0;   // ... the bin count 4..360 and the window radius 0..32
    const float* hprior_table = nullptr;   // heading plans, optional (ccvpe_localize_heading_prior*): the heading prior's tables,
    int hprior_stride = 0, hprior_nb = 0;  //   the floats between two queries' tables (0: one for all) and the table's bins 4..360
    float* cred = nullptr;             // optional [batch][4 + 3 cred_levels] credible rows (ccvpe_*_credible); selects the credible
    int cred_levels = 0;               //   plans; with it the levels 1..8, by value as they travel to the launches,
    float cred_level[CRED_MAX_LEVELS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int32_t* cred_probe = nullptr;       //   the optional probe cell of each query [batch] and
    unsigned char* cred_map = nullptr;         //   the optional level maps [batch][512*512]
    // the view of the micro-batch that starts at query `done`: every per-query buffer advanced by its own row size
    TailCall at(int done) const {
        const size_t d = (size_t)done, npx = (size_t)CCVPE_OUT_HW * CCVPE_OUT_HW;
        TailCall t = *this;
        if (rows) t.rows += d * (topk_k > 0 ? topk_k : 1) * 5;
        if (log_prior) t.log_prior += d * prior_stride;
        if (stats) t.stats += d * 2;
        if (posterior) t.posterior += d * npx;
        if (summary) t.summary += d * SUMMARY_COLS;
        if (heading) { t.heading += d * HEADING_COLS; t.hist += d * heading_bins; }
        if (hprior_table) t.hprior_table += d * hprior_stride;
        if (cred) t.cred += d * (4 + 3 * cred_levels);
        if (cred_probe) t.cred_probe += d;
        if (cred_map) t.cred_map += d * npx;
        return t;
    }
};
static_assert(TAIL_HW == CCVPE_OUT_HW, "the output-side kernels' map side");
// Working memory of the tail for B queries: a plan's tensors and ticket ranges (build_plan) or the prior scratch (ccvpe_api.hip).  A
// buffer no launch of the caller reads stays null.
struct TailBuffers {
    const float* logits = nullptr;     // [B][512*512]
    const float* ori = nullptr;        // [B][2][512*512] (pose.heading)
    float* partial = nullptr;          // [B][64][2] softmax partials
    void* keys = nullptr;              // argmax: [B][64][2] (max, index) pairs; top-K: [B][64][k] 64-bit keys
    int* index = nullptr;              // [B] argmax; top-K: [B][k]
    double* summ_part = nullptr;       // [B][64][SUMMARY_PART] (summary forms)
    double* head_part = nullptr;       // [B][64][HEADING_PART] and
    unsigned long long* bins = nullptr;   //   [B][HEADING_MAX_BINS], zero between launches (pose.heading)
    unsigned* tickets = nullptr;       // [B] counters of pose.argmax or topk.peaks ...
    unsigned* head_tickets = nullptr;  // ... and of pose.heading (the same range where both run in order on one stream)
    unsigned* cred_tickets = nullptr;  // ... and of pose.credible, with
    void* cred_zero = nullptr;         //   its histograms and probe sums (credible_zero_words: zero between launches) and
    void* cred_state = nullptr;        //   the states its passes hand on (credible_state_words)
};
void issue_softmax_partial(const TailBuffers& w, const TailCall& t, int B, hipStream_t s);
void issue_pose_argmax(const TailBuffers& w, const TailCall& t, int B, hipStream_t s);
void issue_topk_peaks(const TailBuffers& w, const TailCall& t, int B, hipStream_t s);
void issue_pose_heading(const TailBuffers& w, const TailCall& t, int B, hipStream_t s);
void issue_pose_credible(const TailBuffers& w, const TailCall& t, const float* belief, int B, hipStream_t s);   // belief: a stored map instead of w.logits

struct Ctx {
    float* arena = nullptr;
    const std::vector<size_t>* off = nullptr;
    hipStream_t stream = nullptr;
    const float* grd = nullptr;
    const float* sat = nullptr;
    ccvpe_outputs out{};
    float* splitk_scratch = nullptr;
    size_t splitk_floats = 0;
    unsigned* tickets = nullptr;       // the plan's last-arriver counters (ticket.h); every launch that draws tickets owns a range
    const float* cache_in = nullptr;   // aerial cache consumed by a "cached" plan
    float* cache_out = nullptr;        // aerial cache produced by an "encode" plan
    TailCall tail;                     // pose plans: what this micro-batch asks of the tail, its own slice of every per-query buffer
    const int* tile_index = nullptr;   // indexed cached forms: HOST tile of each sample of this micro-batch (null: sample b reads tile b)
    int n_tiles = 0;                   // ... and the number of tiles cache_in was encoded for (its section layout)
    const float* grd_cache_in = nullptr;   // pair plans (ccvpe_localize_region): ground cache of ccvpe_encode_ground, [n_queries][Ltot]
    const int* query_index = nullptr;  // ... HOST query of each pair of this micro-batch
    int n_queries = 0;                 // ... and the number of queries grd_cache_in holds
    float* ptr(const Tensor& t) const { return arena + (*off)[t.id]; }
    Dst dst(const Tensor& t, int coff = 0) const { return Dst{ptr(t), t.C, coff, t.split ? 1 : 0, t.numel()}; }
    mutable int conv_errors = 0;   // launches refused by launch_conv_igemm (unsupported geometry)
    mutable size_t conv_tick_off = 0;   // ticket range of the convolution launch being issued (set by Plan::add_conv's wrapper)
    mutable ConvParams* probe = nullptr;   // autotune_plan: the launch is not issued, its parameters are copied here
    void launch_conv(ConvParams& p, int cfg) const {
        p.tickets = tickets ? tickets + conv_tick_off : nullptr;
        p.partial = splitk_scratch;
        p.partial_floats = splitk_floats;
        if (probe) { *probe = p; return; }
        if (launch_conv_igemm(p, cfg, stream) != 0) ++conv_errors;
    }
};

// What selects a plan: one key from the call descriptor (ForwardCall) through get_plan's lookup to build_plan
struct PlanKey {
    int B = 0, gh = 0, gw = 0;
    int mode = 0;                 // 0 full forward, 1 aerial encode only, 2 forward from a cached aerial encoding, 3 ground encode only,
                                  // 4 pose plan from both caches (the pairs of ccvpe_localize_region)
    bool pose = false;            // modes 0 / 2: the pose plan of ccvpe_localize - result rows instead of the nine outputs (build_plan)
    bool topk = false;            // pose plans: the top-K tail of ccvpe_localize_topk (K and r per call, workspace for K = 64)
    bool summary = false;         // argmax pose plans: pose.argmax also writes the summary rows (ccvpe_localize_summary*); the only plans whose
                                  // workspace holds the float64 hand-off of the chunks' sums
    bool heading = false;         // argmax pose plans: the whole orientation field in the workspace and the pose.heading launch behind both
                                  // decoders (ccvpe_localize_heading*); combines with summary
    bool hprior = false;          // heading plans: the combined prior map `comb` in the workspace, written by pose.hprior from the orientation
                                  // field, read by the tail in place of the caller's prior (ccvpe_localize_heading_prior*); needs heading
    bool credible = false;        // argmax pose plans: the pose.credible launches behind pose.argmax, over the logits the workspace still holds
                                  // (ccvpe_localize_credible*); combines with none of topk, summary, heading
    bool operator==(const PlanKey& o) const {
        return B == o.B && gh == o.gh && gw == o.gw && mode == o.mode && pose == o.pose && topk == o.topk && summary == o.summary &&
               heading == o.heading && hprior == o.hprior && credible == o.credible;
    }
};

// One call of the forward family (run_forward, ccvpe_api.hip): every extern "C" entry point checks its own arguments, fills the fields
// it has by name and leaves the rest at their defaults.  The fields that are set select the plan (plan_key) and what each slice's Ctx gets.
struct ForwardCall {
    const float* grd = nullptr;        // ground images [batch][3][gh][gw]
    int gh = 0, gw = 0;
    const float* sat = nullptr;        // full forms: aerial images [batch][3][512][512] (mode 0 plans) ...
    const float* cache = nullptr;      // ... cached forms: the aerial cache of ccvpe_encode_aerial instead (mode 2 plans)
    const int32_t* tile_index = nullptr;   // indexed cached forms: HOST tile of each sample (null: sample b reads tile b, batch <= micro_batch) ...
    int n_tiles = 0;                   // ... and the tiles the cache holds (range of tile_index checked by the entry point)
    int batch = 0;
    const ccvpe_outputs* out = nullptr;   // the nine outputs, or ...
    TailCall tail;                     // ... pose plans (ccvpe_localize*): tail.rows set, `out` is not read; the whole batch's buffers
    hipStream_t stream = nullptr;
    bool profile = false;              // ccvpe_profile_forward: a hipEvent pair around every launch
    PlanKey plan_key() const {         // (B: set per slice by the micro-batch loop)
        PlanKey key;
        key.gh = gh; key.gw = gw; key.mode = cache ? 2 : 0; key.pose = tail.rows != nullptr; key.topk = tail.rows && tail.topk_k > 0;
        key.summary = tail.rows && tail.summary;
        key.heading = tail.rows && tail.heading;
        key.hprior = key.heading && tail.hprior_table;
        key.credible = tail.rows && tail.cred;
        return key;
    }
};

struct Op {
    std::string name;
    std::function<void(const Ctx&)> fn;
    std::vector<int> uses;
    double flops = 0, bytes = 0;
    // implicit-GEMM launches: tile id the launch uses (0 = heuristic) - set by Plan::autotune
    std::shared_ptr<int> tile;
    const char* form = nullptr;   // a launch that is not a tiled GEMM but runs one's arithmetic: the tile part of its profile row ("name|form")
    int gemm_m = 0, gemm_n = 0, gemm_kpad = 0;
    int conv_cin = 0;             // 3x3 layers: input channels (issued-FLOP accounting of the Winograd tiles)
    bool bf16x3_only = false;     // the launch reads a pre-split bf16 tensor: exact-fp32 tiles cannot serve it
    bool wino_ok = false;         // 3x3 / stride 1 layer with Winograd-domain weights packed
    bool wino4_ok = false;        // ... with the F(4x4,3x3) weights packed as well
    bool wino4x_ok = false;       // ... with the xi-split F(4x4,3x3) weights packed
    bool is_pw = false;           // 1x1 conv / k2s2 transposed conv: the pointwise persistent tiles may serve it
    bool proj_ok = false;         // gated project conv with the fragment-order weights packed (kernels_proj.hip)
    // two-stream execution (Plan::schedule): stream the op is issued on, ops of the other stream it must wait for,
    // and whether an op of the other stream waits for this one (then an event is recorded after it)
    int stream = 0;
    std::vector<int> wait_on;
    bool signal = false;
};

struct TapInfo { Tensor t; int coff; int C; };

struct Plan {
    PlanKey key;
    bool debug = false;
    std::vector<size_t> size;     // floats per tensor
    std::vector<size_t> off;      // float offset in the arena
    std::vector<Op> ops;
    std::map<std::string, TapInfo> taps;
    size_t total = 0;             // floats
    float* arena = nullptr;
    Tensor scratch;               // split-K slab scratch shared by every conv launch (whole-plan lifetime)
    // hipGraph replay (latency mode): static staging copies of the inputs / outputs so the captured kernel
    // arguments never change; the caller's buffers are reached by D2D copies outside the graph
    bool use_graph = false;
    Tensor io_grd, io_sat, io_logits, io_heat, io_ori, io_ms[6];
    Tensor tune_cache;            // encode plans: stand-in for the caller's cache while the plan is being autotuned
    hipGraphExec_t exec = nullptr;
    int runs = 0;
    // last-arriver tickets (ticket.h): one device allocation per plan, outside the arena (the autotuner fills the arena with random
    // numbers, and plans share it), zeroed once when the plan is built - every kernel leaves its counters at zero
    size_t ticket_words = 0;
    unsigned* tickets = nullptr;
    size_t alloc_tickets(size_t n) { const size_t o = ticket_words; ticket_words += (n + 15) & ~(size_t)15; return o; }
    int l6_wm = 0;                // composed level 6: the Winograd form its launches run (0: the three launches); get_plan derives the weights
    int l6_split = 0;             // SPLIT6_* bits: the level-6 layers that run in split form (get_plan derives their weights)
    bool tiles_checked = false;   // the first issue compared every tiled launch with its plan entry (ccvpe_api.hip: check_issued_tile)
    // Two-stream execution: the aerial encoder and the orientation decoder are issued on a second stream, so the
    // ramp-up / drain of the ~330 short kernels of one chain is filled by the other chain.  Dependencies come from
    // the ops' tensor lists (any two ops that touch the same tensor stay ordered), and a two-stream plan gives every
    // tensor its own memory (lifetime-based reuse would add hidden dependencies between the streams).
    bool two_streams = false;
    Tensor scratch2;              // split-K slab scratch of the second stream
    std::vector<hipEvent_t> events;   // one per signalling op + fork + join, created on first use
    std::vector<int> issue_order;     // two-stream plans: the order the launches are handed to the two streams (schedule())
    bool issue_interleaved = true, log_schedule = false, no_reuse = false;   // the handle's switches of the same names (build_plan)
    ~Plan() {
        if (exec) (void)hipGraphExecDestroy(exec);
        for (hipEvent_t e : events) if (e) (void)hipEventDestroy(e);
        if (tickets) (void)hipFree(tickets);
    }
    void schedule() {
        if (!two_streams) return;
        bool any = false;
        for (auto& o : ops) {
            o.stream = (o.name.rfind("sat.", 0) == 0 || o.name.rfind("ori", 0) == 0) ? 1 : 0;
            any = any || o.stream == 1;
            o.wait_on.clear();
            o.signal = false;
        }
        if (!any) { two_streams = false; return; }
        std::map<int, int> last_use;   // tensor id -> most recent op that touches it
        for (int i = 0; i < (int)ops.size(); ++i) {
            int dep = -1;              // stream order already covers earlier ops of a stream: the latest one is enough
            for (int id : ops[i].uses) {
                auto it = last_use.find(id);
                if (it != last_use.end() && ops[it->second].stream != ops[i].stream) dep = std::max(dep, it->second);
            }
            if (dep >= 0) { ops[i].wait_on.push_back(dep); ops[dep].signal = true; }
            for (int id : ops[i].uses) last_use[id] = i;
        }
        // Issue order (round 4).  In plan order every launch of the ground encoder is issued before the first launch of the aerial encoder:
        // the host (eagerly: ~3-4 us per launch; a replayed hipGraph submits its nodes in creation order just the same) feeds the second
        // stream only after ~60 launches of the first, and at batch 1 - where the GPU finishes a launch in 5-20 us - the aerial chain, the
        // one the decoders wait for, started ~450 us late (rocprofv3 timeline of a replayed frame).  The launches are therefore issued
        // interleaved: always the stream that is behind (by the number of launches issued), never ahead of a cross-stream dependency.
        // Any interleaving that keeps each stream's own order and issues a producer before its cross-stream consumer is valid: the
        // streams' memory pools are recycled in stream order, cross-stream tensors keep private memory (assign()).
        issue_order.clear();
        {
            std::vector<int> q[2];
            for (int i = 0; i < (int)ops.size(); ++i) q[ops[i].stream].push_back(i);
            size_t p[2] = {0, 0};
            std::vector<bool> issued(ops.size(), false);
            while (issue_interleaved && (p[0] < q[0].size() || p[1] < q[1].size())) {
                auto ready = [&](int s) {
                    if (p[s] >= q[s].size()) return false;
                    for (int d : ops[q[s][p[s]]].wait_on) if (!issued[d]) return false;
                    return true;
                };
                const bool r0 = ready(0), r1 = ready(1);
                int s;
                if (r0 && r1) s = (p[1] * q[0].size() < p[0] * q[1].size()) ? 1 : 0;   // the stream that has issued the smaller share of its launches
                else if (r0 || r1) s = r0 ? 0 : 1;
                else { issue_order.clear(); break; }                                        // (cannot happen: the dependency graph is acyclic)
                const int i = q[s][p[s]++];
                issued[i] = true;
                issue_order.push_back(i);
            }
            if (issue_order.size() != ops.size()) { issue_order.resize(ops.size()); for (int i = 0; i < (int)ops.size(); ++i) issue_order[i] = i; }
        }
        if (log_schedule)
            for (int i = 0; i < (int)ops.size(); ++i) {
                std::fprintf(stderr, "op %3d s%d %-28s wait=%d uses=", i, ops[i].stream, ops[i].name.c_str(), ops[i].wait_on.empty() ? -1 : ops[i].wait_on[0]);
                for (int id : ops[i].uses) std::fprintf(stderr, "%d ", id);
                std::fprintf(stderr, "\n");
            }
    }
    static constexpr size_t SPLITK_FLOATS = 32u << 20;   // 128 MiB: 16 slabs of M*N <= 2M outputs
    void set_scratch(Ctx& c, int stream) const {         // per-stream scratch pointers of a launch context
        const Tensor& sk = stream ? scratch2 : scratch;
        c.splitk_scratch = c.ptr(sk); c.splitk_floats = SPLITK_FLOATS;
    }

    // every kernel addresses a tensor with 32-bit byte offsets (raw buffer loads, `unsigned in_bytes`, the 0x80000000
    // out-of-range sentinel): no tensor of a plan may reach 2 GiB - checked at the end of build_plan
    size_t max_tensor_bytes = 0;
    int max_dims[4] = {0, 0, 0, 0};
    Tensor alloc(int B_, int H, int W, int C) {
        Tensor t; t.id = (int)size.size(); t.B = B_; t.H = H; t.W = W; t.C = C;
        size.push_back((size_t)B_ * H * W * C);
        if (size.back() * sizeof(float) > max_tensor_bytes) {
            max_tensor_bytes = size.back() * sizeof(float);
            max_dims[0] = B_; max_dims[1] = H; max_dims[2] = W; max_dims[3] = C;
        }
        return t;
    }
    void add(const std::string& name, std::vector<Tensor> uses, std::function<void(const Ctx&)> fn, double flops = 0, double bytes = 0) {
        Op o; o.name = name; o.fn = std::move(fn); o.flops = flops; o.bytes = bytes;
        for (auto& t : uses) o.uses.push_back(t.id);
        ops.push_back(std::move(o));
    }
    void add_conv(const std::string& name, std::vector<Tensor> uses, int gemm_m, int gemm_n, int gemm_kpad,
                  std::function<void(const Ctx&, int)> fn, double flops, double bytes) {
        auto tp = std::make_shared<int>(TILE_AUTO);
        const size_t toff = alloc_tickets(CONV_TICKETS);   // counters of a self-reducing split-K launch (ticket.h)
        add(name, std::move(uses), [fn, tp, toff](const Ctx& c) { c.conv_tick_off = toff; fn(c, *tp); }, flops, bytes);
        ops.back().tile = tp;
        ops.back().gemm_m = gemm_m;
        ops.back().gemm_n = gemm_n;
        ops.back().gemm_kpad = gemm_kpad;
    }
    // Workspace layout.  Single-stream plans: first-fit with lifetime reuse over the program order.  Two-stream plans:
    // memory may only be recycled between tensors whose launches are ordered whichever way the plan is issued - i.e.
    // tensors touched by ONE stream only, recycled among tensors of the same stream (stream order == program order).
    // Tensors that both streams touch (the concat buffers the aerial encoder's taps land in, the descriptor map, the
    // level-1 score stack) keep private memory for the whole plan, so a recycled address never adds a dependency the
    // event edges do not know about.  Three regions: [stream-0 pool | stream-1 pool | cross-stream and pinned tensors].
    void assign() {
        const int n = (int)size.size();
        std::vector<int> first(n, 1 << 30), last(n, -1), smask(n, 0);
        for (int i = 0; i < (int)ops.size(); ++i)
            for (int id : ops[i].uses) {
                first[id] = std::min(first[id], i); last[id] = std::max(last[id], i);
                smask[id] |= 1 << (two_streams ? ops[i].stream : 0);
            }
        std::vector<bool> pinned(n, false);
        auto pin = [&](const Tensor& t) { if (t.id >= 0) { pinned[t.id] = true; first[t.id] = 0; last[t.id] = 1 << 30; } };
        if (debug || no_reuse) for (int i = 0; i < n; ++i) if (last[i] >= 0) pinned[i] = true;
        pin(scratch); pin(scratch2); pin(tune_cache);
        if (use_graph)
            for (const Tensor* t : {&io_grd, &io_sat, &io_logits, &io_heat, &io_ori, &io_ms[0], &io_ms[1], &io_ms[2], &io_ms[3], &io_ms[4], &io_ms[5]}) pin(*t);
        for (int i = 0; i < n; ++i) if (smask[i] == 3) pinned[i] = true;
        off.assign(n, 0);
        std::vector<int> order(n);
        for (int i = 0; i < n; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return first[a] < first[b]; });
        auto granule = [&](int id) { return (size[id] + 63) & ~(size_t)63; };   // 256-byte granules
        total = 0;
        for (int pool = 1; pool <= 2; ++pool) {   // recycled regions of stream 0 and stream 1
            const size_t base = total;
            std::vector<int> placed;
            for (int id : order) {
                if (last[id] < 0 || pinned[id] || smask[id] != pool) continue;
                const size_t sz = granule(id);
                // candidate offsets: the region start and the end of every live, lifetime-overlapping tensor
                std::vector<std::pair<size_t, size_t>> busy;
                for (int o : placed)
                    if (!(last[o] < first[id] || last[id] < first[o])) busy.push_back({off[o], off[o] + granule(o)});
                std::sort(busy.begin(), busy.end());
                size_t pos = base;
                for (auto& iv : busy) {
                    if (pos + sz <= iv.first) break;
                    pos = std::max(pos, iv.second);
                }
                off[id] = pos;
                total = std::max(total, pos + sz);
                placed.push_back(id);
            }
        }
        for (int id : order) {   // private memory
            if (last[id] < 0 || !pinned[id]) continue;
            off[id] = total;
            total += granule(id);
        }
    }
};

struct ccvpe_handle_s {
    ccvpe_config cfg{};
    VariantSpec vs{};
    int rolls[6] = {0};                               // R_k of the ms outputs
    std::map<std::string, std::vector<int64_t>> expect;   // key -> shape
    std::map<std::string, std::vector<float>> host;       // raw host copies until finalize
    std::set<std::string> skipped;
    bool finalized = false;
    bool debug = false;
    Switches sw;                  // environment switches, read at ccvpe_create
    hipStream_t capture_stream = nullptr;
    hipStream_t aux_stream = nullptr;   // second stream of two-stream plans
    bool serial_issue = false;    // ccvpe_set_streams(h, 1): run two-stream plans in program order on one stream
    std::vector<void*> dev_allocs;
    std::vector<size_t> dev_alloc_bytes;   // parallel to dev_allocs (packed-weight cache: ccvpe_save_packed)
    EncoderW grd_enc, sat_enc;
    PackedConv grd_heads, sat_desc;
    float* grd_wh[6] = {nullptr};
    float grd_b2[6] = {0};
    DecoderW loc, ori;
    Level6W l6[2];                // loc, ori (ensure_level6)
    int l6_wm = 0;                // the Winograd form l6 was derived for (0: not derived)
    std::vector<void*> l6_allocs;
    bool l6_failed = false;       // the derivation failed once (out of memory): plans under the automatic rule keep the three launches
    bool l6_split = false;        // l6[.].wb / ws are derived (ensure_level6_split)
    bool l6_split_failed = false; // ... failed once: plans under the automatic rule keep the tiled launches
    std::vector<std::unique_ptr<Plan>> plans;
    Plan* last_plan = nullptr;    // plan of the most recent forward (ccvpe_debug_dump_plan)
    float* snap[2] = {nullptr, nullptr};   // CCVPE_DIAG_SNAP: the named launch's tensors before / after it
    size_t snap_floats = 0;
    std::vector<std::pair<int, size_t>> snap_layout;   // (tensor id, float offset inside a snapshot buffer)
    std::map<std::pair<int, int>, int> mb_cap;   // ground size -> ccvpe_max_micro_batch (2 GiB tensor bound)
    // tuning table (ccvpe_tune.hip): launch key -> (tile name, split-K code); launches found here are not measured again
    std::map<std::string, std::pair<std::string, int>> tuning;
    int tuned_plans = 0;          // plans this handle has (partly) tuned by measurement (ccvpe_tuning_generation)
    float* arena = nullptr;
    size_t arena_floats = 0;
    // Growable scratch of the four post-processing families (ensure_scratch, ccvpe_api.hip).  One buffer each: the families may be in
    // flight on different streams of one handle at once, and every buffer carries its own ticket counters.
    struct Scratch { void* ptr = nullptr; int batch = 0; };
    Scratch post_scratch;         // launch_postprocess: partial pairs and ticket counters
    Scratch topk_scratch;         // ccvpe_postprocess_topk: ticket counters, hand-off keys and indices
    Scratch prior_scratch;        // ccvpe_postprocess_prior, ccvpe_track_update_logits, ccvpe_postprocess_summary, ccvpe_belief_summary: the
                                  // top-K scratch plus softmax partials plus the summary's float64 hand-off plus, for ccvpe_postprocess_heading,
                                  // the heading sums' hand-off and the queries' fixed-point histograms
    Scratch joint_scratch;        // ccvpe_track_joint_update_logits: softmax partials and the chunks' hand-offs (track_joint_scratch_bytes)
    // profiling rows of the last ccvpe_profile_forward
    struct Row { std::string name; float ms; double flops, bytes, issued; };
    std::vector<Row> prof;
};


// ---- ccvpe_weights.hip ----
void build_expect(ccvpe_handle_s* h);
int pack_conv(ccvpe_handle_s* h, PackedConv& pc, int N, int taps, int cin, int cinp, const std::vector<int>& cmap,
              const std::function<float(int, int, int)>& get, const std::vector<float>& bias, int KH, int KW);
std::vector<int> identity_map(int n);
static inline int score_pad(int nscore) { return round_up(nscore, 8); }

// ---- ccvpe_plan.hip ----
ConvParams conv_params(const PackedConv& pc, const float* in, int in_ld, int B, int H, int W, int OH, int OW,
                       int stride, int pad_t, int pad_l, int act);
size_t cache_layout(const VariantSpec& vs, int B, size_t off[6]);
int ground_desc_floats(const ccvpe_handle_s* h, int gh, int gw);   // Ltot of a ground image (ground cache row), < 0: bad geometry
int build_plan(ccvpe_handle_s* h, Plan& pl, const PlanKey& key);
// the fused last level's parameters from a decoder's composed weights, at 512 x 512; the caller adds x, out, raw, tile, max_wg
Level1Params level1_params(const DecoderW& dw, int x_ld, int B, int cout, bool normalize);

// ---- ccvpe_tune.hip ----
int autotune_plan(ccvpe_handle_s* h, Plan& pl, const std::vector<bool>* known = nullptr);
int get_plan(ccvpe_handle_s* h, const PlanKey& key, Plan** out);
std::string tuning_key(ccvpe_handle_s* h, const Plan& pl, const Op& op);
