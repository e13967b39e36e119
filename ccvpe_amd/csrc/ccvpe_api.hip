// C ABI of libccvpe_hip.so: handle, state_dict ingestion (BN folding + weight packing), execution
// plan with lifetime-based workspace reuse, forward orchestration.  See include/ccvpe.h.
//
// The orchestration restates CVM_*.forward (reference models.py:150-343, 448-652, 752-950, 1051-1244)
// as a static list of kernel launches over NHWC tensors; concatenations are channel-offset writes
// into pre-allocated buffers, the encoder taps are written by the producing GEMM's epilogue.
#include "ccvpe_internal.h"

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
namespace ccvpe { thread_local unsigned long long g_launches = 0; }
static thread_local std::string g_err_storage;
std::string& ccvpe_err() { return g_err_storage; }
int ccvpe_fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err_storage = buf;
    return code;
}

// Integer checksum of a tensor's bytes (diagnostics: ccvpe_debug_dump_plan)
__global__ __launch_bounds__(256) void checksum_kernel(const uint32_t* __restrict__ p, size_t n, unsigned long long* out) {
    unsigned long long s = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) s += (unsigned long long)p[i] * (unsigned long long)((i & 1023) + 1);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, s);
}


// ------------------------------------------------------------------------------------------------
// environment switches: the library's only reader of the environment (INTEGRATION.md lists the variables)
// ------------------------------------------------------------------------------------------------
Switches read_switches() {
    Switches s;
    auto set = [](const char* name) { return getenv(name) != nullptr; };
    auto off = [](const char* name) { const char* e = getenv(name); return e && std::atoi(e) == 0; };   // set to 0
    if (const char* e = getenv("CCVPE_AUTOTUNE")) s.autotune = std::atoi(e) != 0;
    if (const char* e = getenv("CCVPE_FUSE_MBCONV")) s.fuse_mbconv = std::atoi(e);
    if (const char* e = getenv("CCVPE_FUSE_L1")) s.fuse_level1 = std::atoi(e) != 0;
    if (const char* e = getenv("CCVPE_L1_TILE")) s.l1_tile = std::atoi(e);
    if (const char* e = getenv("CCVPE_COMPOSE_L6")) s.compose_l6 = std::atoi(e);
    if (const char* e = getenv("CCVPE_SPLIT_L6")) s.split_l6 = std::atoi(e);
    if (const char* e = getenv("CCVPE_DECONV_K2S2")) s.deconv_k2s2 = std::atoi(e);
    if (const char* e = getenv("CCVPE_WINOGRAD")) s.wino = std::atoi(e) != 0;
    if (const char* e = getenv("CCVPE_GRAPH")) s.graph_mode = std::atoi(e) != 0;
    if (const char* e = getenv("CCVPE_STREAMS")) s.two_streams = std::atoi(e) >= 2;
    if (const char* e = getenv("CCVPE_PRECISION")) s.precision = (std::string(e) == "bf16x3") ? 1 : 0;
    s.stem_dw = !off("CCVPE_STEM_DW");
    if (const char* e = getenv("CCVPE_FRONT_SPREAD")) s.front_spread = std::atoi(e);
    s.mbconv_image = !off("CCVPE_MBCONV_IMAGE");
    s.se_ticket = !off("CCVPE_SE_TICKET");
    if (const char* e = getenv("CCVPE_SE_PROLOGUE")) s.se_prologue = std::atoi(e) == 1;
    s.split_planes = !set("CCVPE_NO_SPLIT_PLANES");
    s.match_prep_early = !off("CCVPE_MATCH_PREP_EARLY");
    s.match_wide = !off("CCVPE_MATCH_WIDE");
    s.issue_interleaved = !off("CCVPE_ISSUE_ORDER");
    s.log_schedule = set("CCVPE_LOG_SCHEDULE");
    s.no_reuse = set("CCVPE_NO_REUSE");
    s.tune_prefer_pw = set("CCVPE_TUNE_PREFER_PW");
    if (const char* e = getenv("CCVPE_TUNE_PREFER_PROJ")) { s.tune_prefer_proj = true; s.tune_prefer_lat = std::strcmp(e, "lat") == 0; }
    if (const char* e = getenv("CCVPE_TUNE_SPLITK")) s.tune_splitk = std::atoi(e);
    s.tune_no_bf16x3 = set("CCVPE_TUNE_NO_BF16X3");
    s.no_pw = set("CCVPE_NO_PW");
    s.tune_ignore_table = set("CCVPE_TUNE_IGNORE_TABLE");
    s.tune_lat_rows = set("CCVPE_TUNE_LAT_ROWS");
    s.tune_lat_split = set("CCVPE_TUNE_LAT_SPLIT");
    s.tune_no_fused_split = set("CCVPE_TUNE_NO_FUSED_SPLIT");
    if (const char* e = getenv("CCVPE_TUNE_VERBOSE")) s.tune_verbose = e;
    s.no_proj = set("CCVPE_NO_PROJ");
    if (const char* e = getenv("CCVPE_WINO4_MIN_N")) s.wino4_min_n = std::atoi(e);
    s.no_wino4 = set("CCVPE_NO_WINO4");
    s.no_wino4x = set("CCVPE_NO_WINO4X");
    s.pad_concat = !off("CCVPE_PAD_CONCAT");
    if (const char* e = getenv("CCVPE_DIAG_SYNC_BEFORE")) s.diag_sync = e;
    if (const char* e = getenv("CCVPE_DIAG_SNAP")) s.diag_snap = e;
    return s;
}

// Largest micro-batch whose plan keeps every tensor below 2 GiB, under the switches `sw`.  A device-less stand-in handle: build_plan
// only sizes tensors and records launches, it never touches HIP.  fuse_mbconv = 0 sizes the unfused (largest) form of every MBConv
// block, fuse_level1 = false the unfused last decoder level (a handle may run with CCVPE_FUSE_L1=0 or a level-1 input the fused kernel
// does not take), so the bound holds whatever flags the real handle has.
static int max_micro_batch(const Switches& sw, int variant, float ori_noise, int grd_h, int grd_w) {
    if (variant < 0 || variant > 3) return ccvpe_fail(CCVPE_EINVAL, "unknown variant %d", variant);
    ccvpe_handle_s tmp;
    tmp.cfg.variant = variant; tmp.cfg.ori_noise = ori_noise; tmp.cfg.micro_batch = 1;
    tmp.vs = make_variant(variant);
    tmp.sw = sw;
    tmp.sw.fuse_mbconv = 0; tmp.sw.fuse_level1 = false; tmp.sw.two_streams = false; tmp.sw.graph_mode = 0;
    const int n = (int)(ori_noise / 18.f);
    for (int k = 0; k < 6; ++k) tmp.rolls[k] = (variant == CCVPE_VARIANT_VIGOR_ORI_PRIOR && k > 0) ? 2 * n + 1 : tmp.vs.n_rolls;
    int lo = 0, hi = 1024;   // invariant: lo fits (0 = nothing fits / bad geometry), hi does not
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        Plan pl;
        PlanKey key;
        key.B = mid; key.gh = grd_h; key.gw = grd_w;
        if (build_plan(&tmp, pl, key) == 0) lo = mid; else hi = mid;
    }
    if (lo == 0) return ccvpe_fail(CCVPE_EINVAL, "ground size %d x %d is not valid for variant %d: %s", grd_h, grd_w, variant, ccvpe_err().c_str());
    return lo;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

const char* ccvpe_last_error(void) { return ccvpe_err().c_str(); }
const char* ccvpe_version(void) { return "ccvpe-hip 0.1 (gfx950, fp32 MFMA)"; }
uint64_t ccvpe_launch_count(void) { return ccvpe::g_launches; }

int ccvpe_create(const ccvpe_config* cfg, ccvpe_handle* out) {
    if (!cfg || !out) return ccvpe_fail(CCVPE_EINVAL, "null argument");
    if (cfg->variant < 0 || cfg->variant > 3) return ccvpe_fail(CCVPE_EINVAL, "unknown variant %d", cfg->variant);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return ccvpe_fail(CCVPE_EHIP, "no HIP device visible: libccvpe_hip has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return ccvpe_fail(CCVPE_EINVAL, "device %d out of range (%d visible)", cfg->device, ndev);
    HIPCHK(hipSetDevice(cfg->device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, cfg->device));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        return ccvpe_fail(CCVPE_EHIP, "device %d is %s; this library carries gfx950 code objects only", cfg->device, prop.gcnArchName);
    auto* h = new ccvpe_handle_s();
    h->cfg = *cfg;
    if (h->cfg.micro_batch <= 0) h->cfg.micro_batch = 32;
    h->vs = make_variant(cfg->variant);
    h->sw = read_switches();
    if (h->sw.precision) h->cfg.reserved[0] = *h->sw.precision;
    if (h->cfg.reserved[0] != 0 && h->cfg.reserved[0] != 1) { delete h; return ccvpe_fail(CCVPE_EINVAL, "unknown precision mode %d", cfg->reserved[0]); }
    const int n = (int)(cfg->ori_noise / 18.f);
    for (int k = 0; k < 6; ++k)
        h->rolls[k] = (cfg->variant == CCVPE_VARIANT_VIGOR_ORI_PRIOR && k > 0) ? 2 * n + 1 : h->vs.n_rolls;
    if (cfg->variant == CCVPE_VARIANT_VIGOR_ORI_PRIOR && (n < 0 || 2 * n + 1 > 32)) {
        delete h;
        return ccvpe_fail(CCVPE_EINVAL, "ori_noise %.1f out of range", cfg->ori_noise);
    }
    build_expect(h);
    *out = h;
    return 0;
}

int ccvpe_max_micro_batch(int32_t variant, float ori_noise, int32_t grd_h, int32_t grd_w) {
    return max_micro_batch(read_switches(), variant, ori_noise, grd_h, grd_w);
}

int ccvpe_destroy(ccvpe_handle h) {
    if (!h) return 0;
    (void)hipSetDevice(h->cfg.device);
    for (void* p : h->dev_allocs) (void)hipFree(p);
    release_level6(h);
    if (h->arena) (void)hipFree(h->arena);
    for (auto* buf : {&h->post_scratch, &h->topk_scratch, &h->prior_scratch, &h->joint_scratch}) if (buf->ptr) (void)hipFree(buf->ptr);
    h->plans.clear();
    for (int k = 0; k < 2; ++k) if (h->snap[k]) (void)hipFree(h->snap[k]);
    if (h->capture_stream) (void)hipStreamDestroy(h->capture_stream);
    if (h->aux_stream) (void)hipStreamDestroy(h->aux_stream);
    delete h;
    return 0;
}

int ccvpe_output_channels(ccvpe_handle h, int32_t level) {
    if (!h || level < 0 || level > 5) return ccvpe_fail(CCVPE_EINVAL, "bad level");
    return h->rolls[level];
}

size_t ccvpe_workspace_bytes(ccvpe_handle h, int32_t batch, int32_t grd_h, int32_t grd_w) {
    if (!h || !h->finalized || batch <= 0) { ccvpe_fail(CCVPE_ESTATE, "handle not ready"); return 0; }
    Plan pl;
    PlanKey key;
    key.B = std::min(batch, h->cfg.micro_batch); key.gh = grd_h; key.gw = grd_w;
    if (build_plan(h, pl, key)) return 0;
    return pl.total * sizeof(float);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// forward orchestration (C++ linkage: the micro-batch loop is a template)
// ------------------------------------------------------------------------------------------------
// Issue a plan's ops: in order on one stream, or on two streams with event edges for the cross-stream dependencies.
// First issue of a plan: every tiled launch must run the (tile, split-K) its plan entry names.  launch_conv_igemm falls back to the shape
// heuristic when a tile cannot serve a launch (a hand-edited or foreign tuning table): legal, but then "same table -> same launches ->
// same bits" no longer holds, so it is said out loud once per plan.
static void check_issued_tile(Plan& pl, const Op& op) {
    const int got = conv_tile_last();
    if (!op.tile || (*op.tile & 0xff) == 0 || got == 0) return;
    const int want = *op.tile, ws = (want >> 8) & 0xff, gs = (got >> 8) & 0xff;
    if ((want & 0xff) != (got & 0xff) || (ws > 1 ? ws : 1) != (gs > 1 ? gs : 1))
        std::fprintf(stderr, "ccvpe: launch %s (batch %d) runs %s split %d instead of the planned %s split %d\n", op.name.c_str(), pl.key.B,
                     conv_tile_name(got), gs, conv_tile_name(want), ws);
}

static int run_ops(ccvpe_handle h, Plan& pl, const Ctx& base, hipStream_t s0) {
    const bool check = !pl.tiles_checked;
    pl.tiles_checked = true;
    if (check) (void)conv_tile_last();
    if (!pl.two_streams || h->serial_issue) {
        Ctx c = base;
        c.stream = s0;
        for (auto& op : pl.ops) { op.fn(c); if (check) check_issued_tile(pl, op); }
        base.conv_errors += c.conv_errors;
        return 0;
    }
    if (!h->aux_stream) HIPCHK(hipStreamCreateWithFlags(&h->aux_stream, hipStreamNonBlocking));
    if (pl.events.empty()) {
        pl.events.assign(pl.ops.size() + 2, nullptr);
        for (size_t i = 0; i < pl.events.size(); ++i)
            if (i >= pl.ops.size() || pl.ops[i].signal) HIPCHK(hipEventCreateWithFlags(&pl.events[i], hipEventDisableTiming));
    }
    Ctx c[2] = {base, base};
    hipStream_t st[2] = {s0, h->aux_stream};
    c[0].stream = st[0];
    c[1].stream = st[1];
    pl.set_scratch(c[1], 1);
    const size_t n = pl.ops.size();
    HIPCHK(hipEventRecord(pl.events[n], st[0]));            // fork: the second stream starts after the caller's prior work
    HIPCHK(hipStreamWaitEvent(st[1], pl.events[n], 0));
    for (size_t k = 0; k < n; ++k) {
        const size_t i = pl.issue_order.size() == n ? (size_t)pl.issue_order[k] : k;
        Op& op = pl.ops[i];
        for (int d : op.wait_on) HIPCHK(hipStreamWaitEvent(st[op.stream], pl.events[d], 0));
        if (!h->sw.diag_sync.empty() && op.name.find(h->sw.diag_sync) != std::string::npos) HIPCHK(hipDeviceSynchronize());
        const bool snap = !h->sw.diag_snap.empty() && op.name == h->sw.diag_snap;
        auto take_snap = [&](int which) -> int {
            if (!h->snap[0]) {
                h->snap_layout.clear();
                size_t o = 0;
                for (int id : op.uses) { h->snap_layout.push_back({id, o}); o += (pl.size[id] + 63) & ~(size_t)63; }
                h->snap_floats = o;
                for (int k = 0; k < 2; ++k) HIPCHK(hipMalloc((void**)&h->snap[k], o * sizeof(float)));
            }
            for (auto& e : h->snap_layout)
                HIPCHK(hipMemcpyAsync(h->snap[which] + e.second, base.arena + pl.off[e.first], pl.size[e.first] * sizeof(float), hipMemcpyDeviceToDevice, st[op.stream]));
            return 0;
        };
        if (snap) { if (int r = take_snap(0)) return r; }
        op.fn(c[op.stream]);
        if (check) check_issued_tile(pl, op);
        if (snap) { if (int r = take_snap(1)) return r; }
        if (op.signal) HIPCHK(hipEventRecord(pl.events[i], st[op.stream]));
    }
    HIPCHK(hipEventRecord(pl.events[n + 1], st[1]));        // join
    HIPCHK(hipStreamWaitEvent(st[0], pl.events[n + 1], 0));
    base.conv_errors += c[0].conv_errors + c[1].conv_errors;
    return 0;
}

// Samples per plan of a gh x gw ground image: the handle's micro-batch, lowered so that no plan has a tensor of 2 GiB or more (32-bit
// byte offsets); larger batches loop.
static int micro_batch_cap(ccvpe_handle h, int gh, int gw) {
    int mbmax = h->cfg.micro_batch;
    auto it = h->mb_cap.find({gh, gw});
    if (it == h->mb_cap.end()) {
        const std::string keep = ccvpe_err();
        const int cap = max_micro_batch(h->sw, h->cfg.variant, h->cfg.ori_noise, gh, gw);
        ccvpe_err() = keep;
        it = h->mb_cap.emplace(std::make_pair(gh, gw), cap).first;
    }
    if (it->second > 0) mbmax = std::min(mbmax, it->second);
    return mbmax;
}

// the launches just issued, as "<what> failed: ..." when one of them was refused
static int launch_status(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ccvpe_fail(CCVPE_EHIP, "%s failed: %s", what, hipGetErrorString(e));
    return 0;
}

// launch context of a plan on the caller's stream: the workspace side; the caller adds what the call reads and writes
static Ctx plan_ctx(ccvpe_handle h, const Plan& pl, hipStream_t stream) {
    Ctx c;
    c.arena = h->arena; c.off = &pl.off; c.stream = stream;
    c.tickets = pl.tickets;
    pl.set_scratch(c, 0);
    return c;
}

// The micro-batch loop of the forward family and of ccvpe_localize_region: `total` samples (pairs) in slices of at most micro_batch_cap.
// Two passes: every plan (and the largest arena) exists before the first launch; then slice(pl, c, done, mb) adds the slice's own pointers
// to the plan's launch context and issues it.
template <class Slice>
static int for_each_micro_batch(ccvpe_handle h, PlanKey key, int total, hipStream_t stream, Slice slice) {
    const int mbmax = micro_batch_cap(h, key.gh, key.gw);
    for (int pass = 0; pass < 2; ++pass)
        for (int done = 0; done < total; done += key.B) {
            key.B = std::min(mbmax, total - done);
            Plan* pl;
            if (int rc = get_plan(h, key, &pl)) return rc;
            if (pass == 0) continue;
            h->last_plan = pl;
            Ctx c = plan_ctx(h, *pl, stream);
            if (int rc = slice(pl, c, done, key.B)) return rc;
            if (c.conv_errors) return ccvpe_fail(CCVPE_EINVAL, "%d convolution launches were refused (unsupported geometry)", c.conv_errors);
        }
    return 0;
}

// One slice of a forward call: a replayed hipGraph (latency mode), eager launches, or launch by launch between events (profile)
static int issue_forward(ccvpe_handle h, Plan* pl, Ctx& c, const ForwardCall& fc, int mb) {
    const int gh = fc.gh, gw = fc.gw;
    const bool profile = fc.profile;
    hipStream_t stream = fc.stream;
    const size_t npx = (size_t)CCVPE_OUT_HW * CCVPE_OUT_HW;
    if (!profile && pl->use_graph && !h->debug) {
        // latency mode: stage inputs, replay the captured launch sequence, copy the outputs out
        const ccvpe_outputs user = c.out;
        const float* ugrd = c.grd; const float* usat = c.sat;
        c.grd = c.ptr(pl->io_grd); c.sat = c.ptr(pl->io_sat);
        c.out.logits_flattened = c.ptr(pl->io_logits); c.out.heatmap = c.ptr(pl->io_heat); c.out.ori = c.ptr(pl->io_ori);
        for (int k = 0; k < 6; ++k) c.out.matching_score[k] = c.ptr(pl->io_ms[k]);
        {   // both inputs in one launch (sizes are multiples of 4 floats: 3 x H x W with even H or W - else the runtime copies)
            const size_t ng = (size_t)mb * 3 * gh * gw, ns = (size_t)mb * 3 * CCVPE_SAT_HW * CCVPE_SAT_HW;
            if (ng % 4 == 0 && ((uintptr_t)ugrd % 16) == 0 && ((uintptr_t)usat % 16) == 0) {
                MultiCopy mc{};
                mc.src[0] = ugrd; mc.dst[0] = (float*)c.grd; mc.n[0] = ng;
                mc.src[1] = usat; mc.dst[1] = (float*)c.sat; mc.n[1] = ns;
                mc.count = 2;
                launch_multi_copy(mc, stream);
            } else {
                HIPCHK(hipMemcpyAsync((void*)c.grd, ugrd, ng * sizeof(float), hipMemcpyDeviceToDevice, stream));
                HIPCHK(hipMemcpyAsync((void*)c.sat, usat, ns * sizeof(float), hipMemcpyDeviceToDevice, stream));
            }
        }
        if (!pl->exec && pl->runs >= 1) {   // first call ran eagerly (lazy kernel attributes are set): capture now
            // capture on a private stream (the caller's may be the legacy null stream, which cannot capture)
            hipGraph_t graph = nullptr;
            if (!h->capture_stream) HIPCHK(hipStreamCreateWithFlags(&h->capture_stream, hipStreamNonBlocking));
            HIPCHK(hipStreamBeginCapture(h->capture_stream, hipStreamCaptureModeThreadLocal));
            const int rrc = run_ops(h, *pl, c, h->capture_stream);
            hipError_t ce = hipStreamEndCapture(h->capture_stream, &graph);
            if (rrc) ce = hipErrorUnknown;
            if (ce == hipSuccess && graph) {
                hipGraphExec_t ex = nullptr;
                if (hipGraphInstantiate(&ex, graph, nullptr, nullptr, 0) == hipSuccess) pl->exec = ex;
                (void)hipGraphDestroy(graph);
            }
            if (!pl->exec) { (void)hipGetLastError(); pl->use_graph = false; }   // fall back to eager launches for good
        }
        if (pl->exec) HIPCHK(hipGraphLaunch(pl->exec, stream));
        else if (int rrc = run_ops(h, *pl, c, stream)) return rrc;
        pl->runs++;
        {   // the nine outputs in one launch
            MultiCopy mc{};
            auto add = [&](float* dst, const float* src, size_t n) { mc.src[mc.count] = src; mc.dst[mc.count] = dst; mc.n[mc.count] = n; ++mc.count; };
            add(user.logits_flattened, c.out.logits_flattened, (size_t)mb * npx);
            add(user.heatmap, c.out.heatmap, (size_t)mb * npx);
            add(user.ori, c.out.ori, (size_t)mb * 2 * npx);
            bool aligned = true;
            for (int k = 0; k < 6; ++k) add(user.matching_score[k], c.out.matching_score[k], (size_t)mb * h->rolls[k] * ((size_t)(8 << k) * (8 << k)));
            for (int i = 0; i < mc.count; ++i) aligned = aligned && mc.n[i] % 4 == 0 && ((uintptr_t)mc.dst[i] % 16) == 0 && ((uintptr_t)mc.src[i] % 16) == 0;
            if (aligned) launch_multi_copy(mc, stream);
            else
                for (int i = 0; i < mc.count; ++i) HIPCHK(hipMemcpyAsync(mc.dst[i], mc.src[i], mc.n[i] * sizeof(float), hipMemcpyDeviceToDevice, stream));
        }
    } else if (!profile) {
        if (int rrc = run_ops(h, *pl, c, stream)) return rrc;
    } else {
        hipEvent_t e0, e1;
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        for (auto& op : pl->ops) {
            (void)conv_tile_last();
            HIPCHK(hipEventRecord(e0, stream));
            op.fn(c);
            HIPCHK(hipEventRecord(e1, stream));
            HIPCHK(hipEventSynchronize(e1));
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, e0, e1));
            const int tile = conv_tile_last();
            std::string nm = op.name;
            double issued = op.flops;   // launches that are not tiled GEMMs: issued == algorithmic
            if (const ConvTile* t = conv_tile(tile)) {
                nm += std::string("|") + t->name;
                if ((tile >> 8) == 255) nm += "_tailsplit";
                else if ((tile >> 8) > SPLIT_FUSED) nm += "_splitk" + std::to_string((tile >> 8) - SPLIT_FUSED) + "r";   // r: reduces itself
                else if ((tile >> 8) > 1) nm += "_splitk" + std::to_string(tile >> 8);
                // FLOPs the launch puts on the matrix pipe: M and N padded to the tile, K to the packed depth;
                // Winograd F(2x2,3x3): 16 products per 2x2 output tile and channel pair; bf16x3: three MFMAs per product
                ConvParams q{};
                q.M = op.gemm_m; q.N = op.gemm_n;
                const double util = conv_tile_util(q, *t);
                const double mn_pad = util > 0 ? (double)op.gemm_m * op.gemm_n / util : 0.0;
                if (t->wino_f == 4) issued = 2.0 * mn_pad * 2.25 * ((op.conv_cin + 3) / 4 * 4);   // 36 products per 4x4 tile; k-steps of 4 channels, all-zero ones skipped
                else if (t->wino_f == 2) issued = 2.0 * mn_pad * 4.0 * op.conv_cin;
                else issued = 2.0 * mn_pad * op.gemm_kpad * (t->family == TILE_BF16X3 ? 3.0 : 1.0);
            } else if (op.form) {
                nm += std::string("|") + op.form;
            }
            h->prof.push_back({nm, ms, op.flops, op.bytes, issued});
        }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
    return 0;
}

static int run_forward(ccvpe_handle h, const ForwardCall& fc) {
    const PlanKey key = fc.plan_key();
    const int batch = fc.batch;
    if (!h || !fc.grd || (!fc.sat && !fc.cache) || (!fc.out && !key.pose)) return ccvpe_fail(CCVPE_EINVAL, "null argument");
    if (fc.cache && !fc.tile_index && batch > h->cfg.micro_batch) return ccvpe_fail(CCVPE_EINVAL, "cached forward needs batch <= micro_batch (%d)", h->cfg.micro_batch);
    if (fc.tile_index && fc.n_tiles > h->cfg.micro_batch)
        return ccvpe_fail(CCVPE_EINVAL, "n_tiles %d exceeds micro_batch (%d), the most ccvpe_encode_aerial writes", fc.n_tiles, h->cfg.micro_batch);
    if (!h->finalized) return ccvpe_fail(CCVPE_ESTATE, "ccvpe_finalize_weights has not been called");
    if (key.pose && h->debug) return ccvpe_fail(CCVPE_ESTATE, "pose plans carry no debug taps: ccvpe_set_debug(h, 0) before ccvpe_localize");
    if (batch <= 0) return ccvpe_fail(CCVPE_EINVAL, "batch must be positive");
    if (!key.pose) {
        if (!fc.out->logits_flattened || !fc.out->heatmap || !fc.out->ori) return ccvpe_fail(CCVPE_EINVAL, "null output buffer");
        for (int k = 0; k < 6; ++k) if (!fc.out->matching_score[k]) return ccvpe_fail(CCVPE_EINVAL, "null matching_score[%d]", k);
    }
    HIPCHK(hipSetDevice(h->cfg.device));
    if (fc.profile) h->prof.clear();
    const size_t npx = (size_t)CCVPE_OUT_HW * CCVPE_OUT_HW;
    auto slice = [&](Plan* pl, Ctx& c, int done, int mb) {
        c.cache_in = fc.cache;
        if (fc.tile_index) { c.tile_index = fc.tile_index + done; c.n_tiles = fc.n_tiles; }   // every slice reads its own indices of the one cache
        c.grd = fc.grd + (size_t)done * 3 * fc.gh * fc.gw;
        c.sat = fc.sat ? fc.sat + (size_t)done * 3 * CCVPE_SAT_HW * CCVPE_SAT_HW : nullptr;
        c.tail = fc.tail.at(done);
        if (!key.pose) {
            c.out.logits_flattened = fc.out->logits_flattened + done * npx;
            c.out.heatmap = fc.out->heatmap + done * npx;
            c.out.ori = fc.out->ori + done * 2 * npx;
            for (int k = 0; k < 6; ++k) {
                const size_t hw = (size_t)(8 << k) * (8 << k);
                c.out.matching_score[k] = fc.out->matching_score[k] + (size_t)done * h->rolls[k] * hw;
            }
        }
        return issue_forward(h, pl, c, fc, mb);
    };
    if (int rc = for_each_micro_batch(h, key, batch, fc.stream, slice)) return rc;
    return launch_status("kernel launch");
}

// the fields every form of the forward family has; the entry point names the rest
static ForwardCall forward_call(const float* grd, int32_t grd_h, int32_t grd_w, int32_t batch, void* stream) {
    ForwardCall fc;
    fc.grd = grd; fc.gh = grd_h; fc.gw = grd_w; fc.batch = batch; fc.stream = (hipStream_t)stream;
    return fc;
}

extern "C" {

int ccvpe_forward(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const float* sat, int32_t batch,
                  const ccvpe_outputs* out, void* stream) {
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.sat = sat; fc.out = out;
    return run_forward(h, fc);
}

int ccvpe_localize(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const float* sat, int32_t batch, float* rows, void* stream) {
    if (!rows) return ccvpe_fail(CCVPE_EINVAL, "null rows");
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.sat = sat; fc.tail.rows = rows;
    return run_forward(h, fc);
}

// the (k, radius) range of the top-K entry points, checked before the handle is used
static int check_topk_args(int32_t k, int32_t radius) {
    if (k < 1 || k > TOPK_MAX_K) return ccvpe_fail(CCVPE_EINVAL, "k must be in 1 .. %d", TOPK_MAX_K);
    if (radius < 0 || radius > TOPK_MAX_R) return ccvpe_fail(CCVPE_EINVAL, "radius must be in 0 .. %d", TOPK_MAX_R);
    return 0;
}

int ccvpe_localize_topk(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const float* sat, int32_t batch, int32_t k,
                        int32_t radius, float* rows, void* stream) {
    if (!rows) return ccvpe_fail(CCVPE_EINVAL, "null rows");
    if (int rc = check_topk_args(k, radius)) return rc;
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.sat = sat; fc.tail.rows = rows; fc.tail.topk_k = k; fc.tail.topk_r = radius;
    return run_forward(h, fc);
}

int ccvpe_profile_forward(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const float* sat, int32_t batch,
                          const ccvpe_outputs* out, void* stream) {
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.sat = sat; fc.out = out; fc.profile = true;
    if (int rc = run_forward(h, fc)) return rc;
    return (int)h->prof.size();
}

int ccvpe_profile_row(ccvpe_handle h, int32_t i, char* name_buf, size_t name_cap, float* ms, double* flops, double* bytes) {
    if (!h || i < 0 || i >= (int)h->prof.size()) return ccvpe_fail(CCVPE_EINVAL, "row out of range");
    const auto& r = h->prof[i];
    if (name_buf && name_cap) { std::strncpy(name_buf, r.name.c_str(), name_cap - 1); name_buf[name_cap - 1] = 0; }
    if (ms) *ms = r.ms;
    if (flops) *flops = r.flops;
    if (bytes) *bytes = r.bytes;
    return 0;
}

int ccvpe_profile_row_issued(ccvpe_handle h, int32_t i, double* issued_flops) {
    if (!h || i < 0 || i >= (int)h->prof.size() || !issued_flops) return ccvpe_fail(CCVPE_EINVAL, "row out of range");
    *issued_flops = h->prof[i].issued;
    return 0;
}

// Scratch of a post-processing family: grows with the largest batch seen (the only synchronising step, once per size); bytes(cap) is
// its size for cap samples, `what` names it in the out-of-memory message
static int ensure_scratch(ccvpe_handle_s::Scratch& buf, int batch, size_t (*bytes)(int), const char* what) {
    if (batch <= buf.batch) return 0;
    HIPCHK(hipDeviceSynchronize());   // a launch in flight may still use the old buffer
    if (buf.ptr) HIPCHK(hipFree(buf.ptr));
    buf = {};
    const int cap = std::max(batch, 32);
    void* d = nullptr;
    if (hipMalloc(&d, bytes(cap)) != hipSuccess) return ccvpe_fail(CCVPE_ENOMEM, "%s", what);
    HIPCHK(hipMemset(d, 0, bytes(cap)));
    HIPCHK(hipDeviceSynchronize());
    buf = {d, cap};
    return 0;
}

// The top-K scratch (topk_scratch_bytes) and the prior scratch for buf.batch samples: [PP_MAX_BATCH ticket counters][B x 64 x 64 keys]
// [B x 64 indices] and, in the prior scratch only, [B x 64 x 2 softmax partials][B x 64 x 8 float64 sums of the summary forms]
// [B x 64 x 4 float64 sums of the heading form][B x 360 fixed-point histogram bins of the heading form, zero between launches like the
// counters]; the argmax form's (max, index) hand-off pairs use the start of the key area.  Every area is a multiple of 8 bytes long.
static size_t prior_scratch_bytes(int B) {
    return topk_scratch_bytes(B) + (size_t)B * TAIL_CHUNKS * 2 * sizeof(float) + (size_t)B * TAIL_CHUNKS * SUMMARY_PART * sizeof(double) +
           (size_t)B * TAIL_CHUNKS * HEADING_PART * sizeof(double) + (size_t)B * HEADING_MAX_BINS * sizeof(unsigned long long) +
           (credible_zero_words(B) + credible_state_words(B)) * sizeof(unsigned);   // (the credible forms: at most CRED_SLICE queries' worth)
}
// ... as the tail's working memory over the forward outputs the caller holds.  pose.argmax and pose.heading share the one ticket
// range: they run in order on one stream, and each leaves its counters at zero
static TailBuffers scratch_buffers(const ccvpe_handle_s::Scratch& buf, const float* logits, const float* ori) {
    TailBuffers w;
    w.logits = logits; w.ori = ori;
    w.tickets = w.head_tickets = reinterpret_cast<unsigned*>(buf.ptr);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(w.tickets + PP_MAX_BATCH);
    w.keys = keys;
    w.index = reinterpret_cast<int*>(keys + (size_t)buf.batch * TAIL_CHUNKS * TOPK_MAX_K);
    w.partial = reinterpret_cast<float*>(w.index + (size_t)buf.batch * TOPK_MAX_K);
    w.summ_part = reinterpret_cast<double*>(w.partial + (size_t)buf.batch * TAIL_CHUNKS * 2);   // (read by the summary forms alone)
    w.head_part = w.summ_part + (size_t)buf.batch * TAIL_CHUNKS * SUMMARY_PART;               // (these two by the heading form alone)
    w.bins = reinterpret_cast<unsigned long long*>(w.head_part + (size_t)buf.batch * TAIL_CHUNKS * HEADING_PART);
    // the credible forms (the prior scratch alone reaches this far): histograms and probe sums, zero between launches, then the states
    w.cred_tickets = w.tickets;
    w.cred_zero = w.bins + (size_t)buf.batch * HEADING_MAX_BINS;
    w.cred_state = reinterpret_cast<unsigned*>(w.cred_zero) + credible_zero_words(buf.batch);
    return w;
}

static int postprocess_any(ccvpe_handle h, const float* heatmap, const float* ori, int32_t batch, ccvpe_pose* poses, float* rows, void* stream) {
    if (!h || !heatmap || !ori || (!poses && !rows) || batch <= 0 || batch > PP_MAX_BATCH) return ccvpe_fail(CCVPE_EINVAL, "bad argument (batch 1 .. 4096)");
    HIPCHK(hipSetDevice(h->cfg.device));
    static_assert(sizeof(ccvpe_pose) == sizeof(PoseOut), "pose layout");
    if (int rc = ensure_scratch(h->post_scratch, batch, postprocess_scratch_bytes, "post-processing scratch")) return rc;
    launch_postprocess(heatmap, ori, batch, CCVPE_OUT_HW * CCVPE_OUT_HW, reinterpret_cast<PoseOut*>(poses), rows, h->post_scratch.ptr, (hipStream_t)stream);
    return launch_status("postprocess launch");
}

int ccvpe_postprocess(ccvpe_handle h, const float* heatmap, const float* ori, int32_t batch, ccvpe_pose* poses, void* stream) {
    if (!poses) return ccvpe_fail(CCVPE_EINVAL, "bad argument");
    return postprocess_any(h, heatmap, ori, batch, poses, nullptr, stream);
}

int ccvpe_postprocess_rows(ccvpe_handle h, const float* heatmap, const float* ori, int32_t batch, float* rows, void* stream) {
    if (!rows) return ccvpe_fail(CCVPE_EINVAL, "bad argument");
    return postprocess_any(h, heatmap, ori, batch, nullptr, rows, stream);
}

int ccvpe_postprocess_topk(ccvpe_handle h, const float* heatmap, const float* ori, int32_t batch, int32_t k, int32_t radius, float* rows,
                           void* stream) {
    if (!h || !heatmap || !ori || !rows) return ccvpe_fail(CCVPE_EINVAL, "null argument");
    if (int rc = check_topk_args(k, radius)) return rc;
    if (batch <= 0 || batch > PP_MAX_BATCH) return ccvpe_fail(CCVPE_EINVAL, "bad argument (batch 1 .. 4096)");
    HIPCHK(hipSetDevice(h->cfg.device));
    if (int rc = ensure_scratch(h->topk_scratch, batch, topk_scratch_bytes, "top-K post-processing scratch")) return rc;
    const TailBuffers w = scratch_buffers(h->topk_scratch, nullptr, ori);   // (tickets, keys and indices only: the peaks come from the heatmap)
    TopkParams p{};
    p.heat = heatmap; p.logits = nullptr; p.partial = nullptr; p.B = batch; p.k = k; p.r = radius;
    p.keys = reinterpret_cast<unsigned long long*>(w.keys); p.tickets = w.tickets; p.index = w.index; p.rows = rows;
    launch_topk_peaks(p, (hipStream_t)stream);
    launch_topk_gather(ori, w.index, batch, k, CCVPE_OUT_HW * CCVPE_OUT_HW, rows, (hipStream_t)stream);
    return launch_status("postprocess_topk launch");
}

int ccvpe_eval_metrics(ccvpe_handle h, const ccvpe_pose* poses, const float* heatmap, int32_t batch, const int32_t* gt_index,
                       const float* gt_cos_sin, const double* meter_per_pixel, const double* heading_deg, ccvpe_metrics* out, void* stream) {
    if (!h || !poses || !heatmap || !gt_index || !meter_per_pixel || !out || batch <= 0) return ccvpe_fail(CCVPE_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    static_assert(sizeof(ccvpe_metrics) == sizeof(MetricsOut), "metrics layout");
    launch_metrics(reinterpret_cast<const PoseOut*>(poses), heatmap, batch, CCVPE_OUT_HW, CCVPE_OUT_HW * CCVPE_OUT_HW, gt_index, gt_cos_sin,
                   meter_per_pixel, heading_deg, reinterpret_cast<MetricsOut*>(out), (hipStream_t)stream);
    return launch_status("metrics launch");
}

int ccvpe_set_streams(ccvpe_handle h, int32_t n_streams) {
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    if (n_streams != 1 && n_streams != 2) return ccvpe_fail(CCVPE_EINVAL, "n_streams must be 1 or 2");
    const bool serial = n_streams == 1;
    if (serial != h->serial_issue)   // captured graphs embed the issue order: drop them
        for (auto& q : h->plans)
            if (q->exec) { (void)hipGraphExecDestroy(q->exec); q->exec = nullptr; q->runs = 0; }
    h->serial_issue = serial;
    return 0;
}

int ccvpe_set_debug(ccvpe_handle h, int32_t enable) {
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    h->debug = enable != 0;
    return 0;
}

int ccvpe_read_tap(ccvpe_handle h, const char* name, float* host_dst, size_t capacity, size_t* n_out, int32_t shape_out[4]) {
    if (!h || !name || !host_dst) return ccvpe_fail(CCVPE_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    Plan* pl = nullptr;
    for (auto it = h->plans.rbegin(); it != h->plans.rend(); ++it)
        if ((*it)->debug) { pl = it->get(); break; }
    if (!pl) return ccvpe_fail(CCVPE_ESTATE, "no debug plan: call ccvpe_set_debug(h, 1) before forward");
    auto it = pl->taps.find(name);
    if (it == pl->taps.end()) return ccvpe_fail(CCVPE_EKEY, "unknown tap '%s'", name);
    const TapInfo& ti = it->second;
    const Tensor& t = ti.t;
    float* base = h->arena + pl->off[t.id];
    HIPCHK(hipDeviceSynchronize());
    if (ti.C < 0) {   // already NCHW
        const size_t n = (size_t)t.B * t.H * t.W * t.C;
        if (n > capacity) return ccvpe_fail(CCVPE_EINVAL, "tap needs %zu floats", n);
        HIPCHK(hipMemcpy(host_dst, base, n * sizeof(float), hipMemcpyDeviceToHost));
        if (n_out) *n_out = n;
        if (shape_out) { shape_out[0] = t.B; shape_out[1] = t.H; shape_out[2] = t.W; shape_out[3] = t.C; }
        return 0;
    }
    const int hw = t.H * t.W;
    const size_t n = (size_t)t.B * ti.C * hw;
    if (n > capacity) return ccvpe_fail(CCVPE_EINVAL, "tap needs %zu floats", n);
    float* tmp = nullptr;
    HIPCHK(hipMalloc((void**)&tmp, n * sizeof(float)));
    launch_nhwc_to_nchw(base, t.C, ti.coff, ti.C, t.B, hw, tmp, nullptr);
    hipError_t e = hipMemcpy(host_dst, tmp, n * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(tmp);
    if (e != hipSuccess) return ccvpe_fail(CCVPE_EHIP, "tap copy failed: %s", hipGetErrorString(e));
    if (n_out) *n_out = n;
    if (shape_out) { shape_out[0] = t.B; shape_out[1] = ti.C; shape_out[2] = t.H; shape_out[3] = t.W; }
    return 0;
}

size_t ccvpe_aerial_cache_bytes(ccvpe_handle h, int32_t batch) {
    if (!h || batch <= 0) { ccvpe_fail(CCVPE_EINVAL, "bad argument"); return 0; }
    size_t off[6];
    return cache_layout(h->vs, batch, off) * sizeof(float);
}

// ccvpe_encode_aerial and ccvpe_encode_ground: one plan (key) for the whole batch, reading the images through the Ctx field `input`
// names, its last launches writing the caller's cache
static int run_encode(ccvpe_handle h, const PlanKey& key, const char* side, const float* Ctx::*input, const float* img, void* cache,
                      void* stream) {
    if (!h || !img || !cache || key.B <= 0) return ccvpe_fail(CCVPE_EINVAL, "bad argument");
    if (!h->finalized) return ccvpe_fail(CCVPE_ESTATE, "ccvpe_finalize_weights has not been called");
    if (key.B > h->cfg.micro_batch) return ccvpe_fail(CCVPE_EINVAL, "%s encode needs batch <= micro_batch (%d)", side, h->cfg.micro_batch);
    HIPCHK(hipSetDevice(h->cfg.device));
    Plan* pl;
    if (int rc = get_plan(h, key, &pl)) return rc;
    Ctx c = plan_ctx(h, *pl, (hipStream_t)stream);
    c.*input = img; c.cache_out = (float*)cache;
    for (auto& op : pl->ops) op.fn(c);
    if (c.conv_errors) return ccvpe_fail(CCVPE_EINVAL, "%d convolution launches were refused (unsupported geometry)", c.conv_errors);
    return launch_status("kernel launch");
}

int ccvpe_encode_aerial(ccvpe_handle h, const float* sat, int32_t batch, void* cache, void* stream) {
    PlanKey key;
    key.B = batch; key.mode = 1;
    return run_encode(h, key, "aerial", &Ctx::sat, sat, cache, stream);
}

int ccvpe_forward_cached(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache, int32_t batch,
                         const ccvpe_outputs* out, void* stream) {
    if (!cache) return ccvpe_fail(CCVPE_EINVAL, "null cache");
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.cache = (const float*)cache; fc.out = out;
    return run_forward(h, fc);
}

int ccvpe_localize_cached(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache, int32_t batch, float* rows,
                          void* stream) {
    if (!cache) return ccvpe_fail(CCVPE_EINVAL, "null cache");
    if (!rows) return ccvpe_fail(CCVPE_EINVAL, "null rows");
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.cache = (const float*)cache; fc.tail.rows = rows;
    return run_forward(h, fc);
}

int ccvpe_localize_topk_cached(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache, int32_t batch,
                               int32_t k, int32_t radius, float* rows, void* stream) {
    if (!cache) return ccvpe_fail(CCVPE_EINVAL, "null cache");
    if (!rows) return ccvpe_fail(CCVPE_EINVAL, "null rows");
    if (int rc = check_topk_args(k, radius)) return rc;
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.cache = (const float*)cache; fc.tail.rows = rows; fc.tail.topk_k = k; fc.tail.topk_r = radius;
    return run_forward(h, fc);
}

// Arguments of the indexed cached forms, checked before the handle is used: tile_index is host memory, so every entry is read
// here and no launch is issued for a call that names a tile outside the cache.
static int check_indexed_args(const float* grd, const void* cache, int32_t n_tiles, const int32_t* tile_index, int32_t batch,
                              const void* result) {
    if (!grd) return ccvpe_fail(CCVPE_EINVAL, "null grd");
    if (!cache) return ccvpe_fail(CCVPE_EINVAL, "null cache");
    if (!tile_index) return ccvpe_fail(CCVPE_EINVAL, "null tile_index");
    if (!result) return ccvpe_fail(CCVPE_EINVAL, "null output buffer");
    if (n_tiles <= 0) return ccvpe_fail(CCVPE_EINVAL, "n_tiles must be positive, got %d", n_tiles);
    if (batch <= 0) return ccvpe_fail(CCVPE_EINVAL, "batch must be positive");
    for (int32_t b = 0; b < batch; ++b)
        if (tile_index[b] < 0 || tile_index[b] >= n_tiles)
            return ccvpe_fail(CCVPE_EINVAL, "tile_index[%d] = %d is outside 0 .. %d (n_tiles %d)", b, tile_index[b], n_tiles - 1, n_tiles);
    return 0;
}

// ... and of the cached forms whose tile_index may be null: then query b reads tile b - the unindexed cached plan, whose cache holds
// exactly one tile per query
static int check_cached_args(const float* grd, const void* cache, int32_t n_tiles, const int32_t* tile_index, int32_t batch, const void* rows) {
    if (tile_index) return check_indexed_args(grd, cache, n_tiles, tile_index, batch, rows);
    if (!grd) return ccvpe_fail(CCVPE_EINVAL, "null grd");
    if (!cache) return ccvpe_fail(CCVPE_EINVAL, "null cache");
    if (!rows) return ccvpe_fail(CCVPE_EINVAL, "null rows");
    if (n_tiles != batch)
        return ccvpe_fail(CCVPE_EINVAL, "without tile_index the cache holds one tile per query: n_tiles %d != batch %d", n_tiles, batch);
    return 0;
}

int ccvpe_forward_cached_indexed(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache, int32_t n_tiles,
                                 const int32_t* tile_index, int32_t batch, const ccvpe_outputs* out, void* stream) {
    if (int rc = check_indexed_args(grd, cache, n_tiles, tile_index, batch, out)) return rc;
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.cache = (const float*)cache; fc.tile_index = tile_index; fc.n_tiles = n_tiles; fc.out = out;
    return run_forward(h, fc);
}

int ccvpe_localize_cached_indexed(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache, int32_t n_tiles,
                                  const int32_t* tile_index, int32_t batch, float* rows, void* stream) {
    if (int rc = check_indexed_args(grd, cache, n_tiles, tile_index, batch, rows)) return rc;
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.cache = (const float*)cache; fc.tile_index = tile_index; fc.n_tiles = n_tiles; fc.tail.rows = rows;
    return run_forward(h, fc);
}

int ccvpe_localize_topk_cached_indexed(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache,
                                       int32_t n_tiles, const int32_t* tile_index, int32_t batch, int32_t k, int32_t radius, float* rows,
                                       void* stream) {
    if (int rc = check_indexed_args(grd, cache, n_tiles, tile_index, batch, rows)) return rc;
    if (int rc = check_topk_args(k, radius)) return rc;
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.cache = (const float*)cache; fc.tile_index = tile_index; fc.n_tiles = n_tiles; fc.tail.rows = rows; fc.tail.topk_k = k; fc.tail.topk_r = radius;
    return run_forward(h, fc);
}

size_t ccvpe_ground_cache_bytes(ccvpe_handle h, int32_t batch, int32_t grd_h, int32_t grd_w) {
    if (!h || batch <= 0) { ccvpe_fail(CCVPE_EINVAL, "bad argument"); return 0; }
    const int ltot = ground_desc_floats(h, grd_h, grd_w);
    if (ltot <= 0) return 0;
    return (size_t)batch * ltot * sizeof(float);
}

int ccvpe_encode_ground(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, int32_t batch, void* cache, void* stream) {
    PlanKey key;
    key.B = batch; key.gh = grd_h; key.gw = grd_w; key.mode = 3;
    return run_encode(h, key, "ground", &Ctx::grd, grd, cache, stream);
}

// Arguments of ccvpe_localize_region, checked before the handle is used: offsets and tiles are host memory, read here in full.
static int check_region_args(const void* grd_cache, int32_t n_queries, const void* sat_cache, int32_t n_tiles, const int32_t* offsets,
                             const int32_t* tiles, const void* rows, const void* best_pair, const void* pair_rows, const void* pair_stats,
                             const void* tile_prob) {
    if (!grd_cache) return ccvpe_fail(CCVPE_EINVAL, "null grd_cache");
    if (!sat_cache) return ccvpe_fail(CCVPE_EINVAL, "null sat_cache");
    if (!offsets) return ccvpe_fail(CCVPE_EINVAL, "null offsets");
    if (!tiles) return ccvpe_fail(CCVPE_EINVAL, "null tiles");
    if (!rows || !best_pair || !pair_rows || !pair_stats || !tile_prob) return ccvpe_fail(CCVPE_EINVAL, "null output buffer");
    if (n_queries <= 0) return ccvpe_fail(CCVPE_EINVAL, "n_queries must be positive, got %d", n_queries);
    if (n_tiles <= 0) return ccvpe_fail(CCVPE_EINVAL, "n_tiles must be positive, got %d", n_tiles);
    if (offsets[0] != 0) return ccvpe_fail(CCVPE_EINVAL, "offsets[0] = %d, must be 0", offsets[0]);
    for (int32_t g = 0; g < n_queries; ++g)
        if (offsets[g + 1] <= offsets[g])
            return ccvpe_fail(CCVPE_EINVAL, "offsets[%d] = %d does not exceed offsets[%d] = %d: every query needs at least one tile", g + 1,
                              offsets[g + 1], g, offsets[g]);
    const int32_t P = offsets[n_queries];
    for (int32_t p = 0; p < P; ++p)
        if (tiles[p] < 0 || tiles[p] >= n_tiles)
            return ccvpe_fail(CCVPE_EINVAL, "tiles[%d] = %d is outside 0 .. %d (n_tiles %d)", p, tiles[p], n_tiles - 1, n_tiles);
    return 0;
}

// ccvpe_localize_region and, with pair_log_prior set, ccvpe_localize_region_prior (the arguments checked by the caller)
static int run_region(ccvpe_handle h, const void* grd_cache, int32_t n_queries, int32_t grd_h, int32_t grd_w, const void* sat_cache,
                      int32_t n_tiles, const int32_t* offsets, const int32_t* tiles, float* rows, int32_t* best_pair, float* pair_rows,
                      float* pair_stats, float* tile_prob, void* stream, const float* pair_log_prior, long long prior_stride) {
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    if (n_queries > h->cfg.micro_batch)
        return ccvpe_fail(CCVPE_EINVAL, "n_queries %d exceeds micro_batch (%d), the most ccvpe_encode_ground writes", n_queries, h->cfg.micro_batch);
    if (n_tiles > h->cfg.micro_batch)
        return ccvpe_fail(CCVPE_EINVAL, "n_tiles %d exceeds micro_batch (%d), the most ccvpe_encode_aerial writes", n_tiles, h->cfg.micro_batch);
    if (!h->finalized) return ccvpe_fail(CCVPE_ESTATE, "ccvpe_finalize_weights has not been called");
    if (h->debug) return ccvpe_fail(CCVPE_ESTATE, "pose plans carry no debug taps: ccvpe_set_debug(h, 0) before ccvpe_localize_region");
    const int P = offsets[n_queries];
    std::vector<int32_t> query(P);   // query of each pair; copied into the launch arguments as each slice is issued
    for (int g = 0; g < n_queries; ++g)
        for (int p = offsets[g]; p < offsets[g + 1]; ++p) query[p] = g;
    HIPCHK(hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    TailCall pairs;
    pairs.rows = pair_rows; pairs.stats = pair_stats; pairs.log_prior = pair_log_prior; pairs.prior_stride = pair_log_prior ? prior_stride : 0;
    auto slice = [&](Plan* pl, Ctx& c, int done, int) {
        c.cache_in = (const float*)sat_cache; c.tile_index = tiles + done; c.n_tiles = n_tiles;
        c.grd_cache_in = (const float*)grd_cache; c.query_index = query.data() + done; c.n_queries = n_queries;
        c.tail = pairs.at(done);
        return run_ops(h, *pl, c, s);
    };
    PlanKey key;   // (B: set per slice by the micro-batch loop)
    key.gh = grd_h; key.gw = grd_w; key.mode = 4; key.pose = true;
    if (int rc = for_each_micro_batch(h, key, P, s, slice)) return rc;
    launch_region_reduce(pair_stats, pair_rows, offsets, n_queries, rows, best_pair, tile_prob, s);
    return launch_status("kernel launch");
}

int ccvpe_localize_region(ccvpe_handle h, const void* grd_cache, int32_t n_queries, int32_t grd_h, int32_t grd_w, const void* sat_cache,
                          int32_t n_tiles, const int32_t* offsets, const int32_t* tiles, float* rows, int32_t* best_pair, float* pair_rows,
                          float* pair_stats, float* tile_prob, void* stream) {
    if (int rc = check_region_args(grd_cache, n_queries, sat_cache, n_tiles, offsets, tiles, rows, best_pair, pair_rows, pair_stats, tile_prob))
        return rc;
    return run_region(h, grd_cache, n_queries, grd_h, grd_w, sat_cache, n_tiles, offsets, tiles, rows, best_pair, pair_rows, pair_stats,
                      tile_prob, stream, nullptr, 0);
}

// ------------------------------------------------------------------------------------------------
// Localize with a per-query position prior: the pose plans with log_prior added to the logits where softmax.partial,
// pose.argmax and topk.peaks read them - no launch of their own.
// ------------------------------------------------------------------------------------------------
// the stride between two queries' prior maps: one shared map or one map each
static int check_prior_stride(int64_t prior_stride) {
    const int64_t n = (int64_t)CCVPE_OUT_HW * CCVPE_OUT_HW;
    if (prior_stride != 0 && prior_stride != n)
        return ccvpe_fail(CCVPE_EINVAL, "prior_stride must be 0 (one shared map) or %lld (one map per query), got %lld", (long long)n,
                          (long long)prior_stride);
    return 0;
}

// the prior arguments, checked before the handle is used; k == 0 is the argmax form, which takes no radius
static int check_prior_args(const float* log_prior, int64_t prior_stride, int32_t k, int32_t radius) {
    if (!log_prior) return ccvpe_fail(CCVPE_EINVAL, "null log_prior");
    if (int rc = check_prior_stride(prior_stride)) return rc;
    if (k < 0 || k > TOPK_MAX_K) return ccvpe_fail(CCVPE_EINVAL, "k must be in 0 .. %d, got %d", TOPK_MAX_K, k);
    if (radius < 0 || radius > TOPK_MAX_R) return ccvpe_fail(CCVPE_EINVAL, "radius must be in 0 .. %d, got %d", TOPK_MAX_R, radius);
    if (k == 0 && radius != 0) return ccvpe_fail(CCVPE_EINVAL, "radius %d needs k >= 1: the argmax form (k = 0) takes radius 0", radius);
    return 0;
}

int ccvpe_localize_prior(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const float* sat, int32_t batch,
                         const float* log_prior, int64_t prior_stride, int32_t k, int32_t radius, float* rows, void* stream) {
    if (!grd) return ccvpe_fail(CCVPE_EINVAL, "null grd");
    if (!sat) return ccvpe_fail(CCVPE_EINVAL, "null sat");
    if (!rows) return ccvpe_fail(CCVPE_EINVAL, "null rows");
    if (int rc = check_prior_args(log_prior, prior_stride, k, radius)) return rc;
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.sat = sat; fc.tail.rows = rows; fc.tail.topk_k = k; fc.tail.topk_r = radius; fc.tail.log_prior = log_prior; fc.tail.prior_stride = prior_stride;
    return run_forward(h, fc);
}

int ccvpe_localize_prior_cached_indexed(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache, int32_t n_tiles,
                                        const int32_t* tile_index, int32_t batch, const float* log_prior, int64_t prior_stride, int32_t k,
                                        int32_t radius, float* rows, void* stream) {
    if (int rc = check_cached_args(grd, cache, n_tiles, tile_index, batch, rows)) return rc;
    if (int rc = check_prior_args(log_prior, prior_stride, k, radius)) return rc;
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.cache = (const float*)cache; fc.tile_index = tile_index; fc.n_tiles = n_tiles;
    fc.tail.rows = rows; fc.tail.topk_k = k; fc.tail.topk_r = radius; fc.tail.log_prior = log_prior; fc.tail.prior_stride = prior_stride;
    return run_forward(h, fc);
}

// The logits forms: the tail of a pose plan (build_plan) over forward outputs the caller holds, in the prior scratch - softmax.partial,
// pose.argmax or topk.peaks, the gather, and pose.heading when the call asks for it
static int run_logits_tail(ccvpe_handle h, const float* logits, const float* ori, int batch, const TailCall& t, hipStream_t s) {
    HIPCHK(hipSetDevice(h->cfg.device));
    if (int rc = ensure_scratch(h->prior_scratch, batch, prior_scratch_bytes, "prior post-processing scratch")) return rc;
    const TailBuffers w = scratch_buffers(h->prior_scratch, logits, ori);
    const int n = CCVPE_OUT_HW * CCVPE_OUT_HW;
    issue_softmax_partial(w, t, batch, s);
    if (t.topk_k > 0) {
        issue_topk_peaks(w, t, batch, s);
        launch_topk_gather(ori, w.index, batch, t.topk_k, n, t.rows, s);
    } else {
        issue_pose_argmax(w, t, batch, s);
        launch_pose_gather(ori, w.index, batch, n, t.rows, s);
    }
    if (t.heading) issue_pose_heading(w, t, batch, s);   // (behind pose.argmax on the same stream: its counters are back at zero, its index is written)
    if (t.cred) issue_pose_credible(w, t, nullptr, batch, s);   // (likewise: the partials of softmax.partial are the map's statistics)
    return 0;
}

int ccvpe_postprocess_prior(ccvpe_handle h, const float* logits, const float* ori, int32_t batch, const float* log_prior,
                            int64_t prior_stride, int32_t k, int32_t radius, float* rows, void* stream) {
    if (!logits) return ccvpe_fail(CCVPE_EINVAL, "null logits");
    if (!ori) return ccvpe_fail(CCVPE_EINVAL, "null ori");
    if (!rows) return ccvpe_fail(CCVPE_EINVAL, "null rows");
    if (int rc = check_prior_args(log_prior, prior_stride, k, radius)) return rc;
    if (batch <= 0 || batch > PP_MAX_BATCH) return ccvpe_fail(CCVPE_EINVAL, "batch must be in 1 .. %d, got %d", PP_MAX_BATCH, batch);
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    TailCall t;
    t.rows = rows; t.topk_k = k; t.topk_r = radius; t.log_prior = log_prior; t.prior_stride = prior_stride;
    if (int rc = run_logits_tail(h, logits, ori, batch, t, (hipStream_t)stream)) return rc;
    return launch_status("postprocess_prior launch");
}

// Kernel-level hook: the tail of the plain argmax pose plan (no prior, no posterior, no summary) on logits the caller holds
int ccvpe_op_pose_rows(ccvpe_handle h, const float* logits, const float* ori, int32_t batch, float* rows, void* stream) {
    if (!logits || !ori || !rows) return ccvpe_fail(CCVPE_EINVAL, "null argument");
    if (batch <= 0 || batch > PP_MAX_BATCH) return ccvpe_fail(CCVPE_EINVAL, "batch must be in 1 .. %d, got %d", PP_MAX_BATCH, batch);
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    TailCall t;
    t.rows = rows;
    if (int rc = run_logits_tail(h, logits, ori, batch, t, (hipStream_t)stream)) return rc;
    return launch_status("op_pose_rows launch");
}

int ccvpe_localize_region_prior(ccvpe_handle h, const void* grd_cache, int32_t n_queries, int32_t grd_h, int32_t grd_w, const void* sat_cache,
                                int32_t n_tiles, const int32_t* offsets, const int32_t* tiles, const float* pair_log_prior,
                                int64_t prior_stride, float* rows, int32_t* best_pair, float* pair_rows, float* pair_stats, float* tile_prob,
                                void* stream) {
    if (int rc = check_region_args(grd_cache, n_queries, sat_cache, n_tiles, offsets, tiles, rows, best_pair, pair_rows, pair_stats, tile_prob))
        return rc;
    if (int rc = check_prior_args(pair_log_prior, prior_stride, 0, 0)) return rc;
    return run_region(h, grd_cache, n_queries, grd_h, grd_w, sat_cache, n_tiles, offsets, tiles, rows, best_pair, pair_rows, pair_stats,
                      tile_prob, stream, pair_log_prior, prior_stride);
}

// ------------------------------------------------------------------------------------------------
// Tracking a frame stream.  Update: the argmax pose plans of ccvpe_localize_prior* with the posterior map as a second
// output of pose.argmax - no launch of their own.  Predict: one launch of track_predict_kernel, no plan and no tuning entry.
// ------------------------------------------------------------------------------------------------
// log_prior may be null (the map is then the forward's heatmap); the stride is checked only beside a prior
static int check_track_update_args(const float* log_prior, int64_t prior_stride, const float* rows, const float* posterior) {
    if (!rows) return ccvpe_fail(CCVPE_EINVAL, "null rows");
    if (!posterior) return ccvpe_fail(CCVPE_EINVAL, "null posterior");
    if (log_prior) if (int rc = check_prior_stride(prior_stride)) return rc;
    if (log_prior && (const float*)log_prior == posterior) return ccvpe_fail(CCVPE_EINVAL, "posterior must not alias log_prior");
    return 0;
}

int ccvpe_track_update(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const float* sat, int32_t batch,
                       const float* log_prior, int64_t prior_stride, float* rows, float* posterior, void* stream) {
    if (!grd) return ccvpe_fail(CCVPE_EINVAL, "null grd");
    if (!sat) return ccvpe_fail(CCVPE_EINVAL, "null sat");
    if (int rc = check_track_update_args(log_prior, prior_stride, rows, posterior)) return rc;
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.sat = sat; fc.tail.rows = rows; fc.tail.log_prior = log_prior; fc.tail.prior_stride = log_prior ? prior_stride : 0; fc.tail.posterior = posterior;
    return run_forward(h, fc);
}

int ccvpe_track_update_cached_indexed(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache, int32_t n_tiles,
                                      const int32_t* tile_index, int32_t batch, const float* log_prior, int64_t prior_stride, float* rows,
                                      float* posterior, void* stream) {
    if (int rc = check_cached_args(grd, cache, n_tiles, tile_index, batch, rows)) return rc;
    if (int rc = check_track_update_args(log_prior, prior_stride, rows, posterior)) return rc;
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.cache = (const float*)cache; fc.tile_index = tile_index; fc.n_tiles = n_tiles;
    fc.tail.rows = rows; fc.tail.log_prior = log_prior; fc.tail.prior_stride = log_prior ? prior_stride : 0; fc.tail.posterior = posterior;
    return run_forward(h, fc);
}

int ccvpe_track_update_logits(ccvpe_handle h, const float* logits, const float* ori, int32_t batch, const float* log_prior,
                              int64_t prior_stride, float* rows, float* posterior, void* stream) {
    if (!logits) return ccvpe_fail(CCVPE_EINVAL, "null logits");
    if (!ori) return ccvpe_fail(CCVPE_EINVAL, "null ori");
    if (int rc = check_track_update_args(log_prior, prior_stride, rows, posterior)) return rc;
    if (posterior == logits) return ccvpe_fail(CCVPE_EINVAL, "posterior must not alias logits");
    if (batch <= 0 || batch > PP_MAX_BATCH) return ccvpe_fail(CCVPE_EINVAL, "batch must be in 1 .. %d, got %d", PP_MAX_BATCH, batch);
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    TailCall t;
    t.rows = rows; t.log_prior = log_prior; t.prior_stride = log_prior ? prior_stride : 0; t.posterior = posterior;
    if (int rc = run_logits_tail(h, logits, ori, batch, t, (hipStream_t)stream)) return rc;
    return launch_status("track_update_logits launch");
}

// The arguments the predict steps share (ccvpe_track_predict, ccvpe_track_predict_affine, ccvpe_heading_predict), checked in the order
// every one of them always had: the five pointers by their names, then the blur's radius, the taps' stride and the batch.  circle: the
// bins of a blur on the circle, which must not wrap onto itself (0: a blur on the plane)
static int check_predict_ptrs(const void* in, const char* in_name, const void* motion, const char* motion_name, const void* taps,
                              const void* floor, const void* out, const char* out_name) {
    if (!in) return ccvpe_fail(CCVPE_EINVAL, "null %s", in_name);
    if (!motion) return ccvpe_fail(CCVPE_EINVAL, "null %s", motion_name);
    if (!taps) return ccvpe_fail(CCVPE_EINVAL, "null taps");
    if (!floor) return ccvpe_fail(CCVPE_EINVAL, "null floor");
    if (!out) return ccvpe_fail(CCVPE_EINVAL, "null %s", out_name);
    return 0;
}
static int check_predict_blur(int32_t radius, int32_t taps_stride, int32_t batch, int32_t circle = 0) {
    if (radius < 0 || radius > TRACK_MAX_R) return ccvpe_fail(CCVPE_EINVAL, "radius must be in 0 .. %d, got %d", TRACK_MAX_R, radius);
    if (circle && 2 * radius + 1 > circle)
        return ccvpe_fail(CCVPE_EINVAL, "radius %d needs 2 radius + 1 <= nb = %d: the blur must not wrap onto itself", radius, circle);
    if (taps_stride != 0 && taps_stride != radius + 1)
        return ccvpe_fail(CCVPE_EINVAL, "taps_stride must be 0 (one set of taps) or radius + 1 = %d (one per query), got %d", radius + 1,
                          taps_stride);
    if (batch <= 0 || batch > PP_MAX_BATCH) return ccvpe_fail(CCVPE_EINVAL, "batch must be in 1 .. %d, got %d", PP_MAX_BATCH, batch);
    return 0;
}

int ccvpe_track_predict(ccvpe_handle h, const float* belief, int32_t batch, const float* shift, const float* taps, int32_t taps_stride,
                        int32_t radius, const float* floor, float* log_prior, void* stream) {
    if (int rc = check_predict_ptrs(belief, "belief", shift, "shift", taps, floor, log_prior, "log_prior")) return rc;
    if (int rc = check_predict_blur(radius, taps_stride, batch)) return rc;
    if (log_prior == belief) return ccvpe_fail(CCVPE_EINVAL, "log_prior must not alias belief");
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    TrackPredictParams p{};
    p.belief = belief; p.shift = shift; p.taps = taps; p.taps_stride = taps_stride; p.radius = radius; p.floor = floor;
    p.log_prior = log_prior; p.B = batch;
    launch_track_predict(p, (hipStream_t)stream);
    return launch_status("track_predict launch");
}

// The predict step under an affine map per query: always one launch of track_predict_affine_kernel - a pure translation
// is not re-routed to track_predict_kernel; choosing is the caller's business.
int ccvpe_track_predict_affine(ccvpe_handle h, const float* belief, int32_t batch, const double* matrix, const float* taps,
                               int32_t taps_stride, int32_t radius, const float* floor, float* log_prior, void* stream) {
    if (int rc = check_predict_ptrs(belief, "belief", matrix, "matrix", taps, floor, log_prior, "log_prior")) return rc;
    if (int rc = check_predict_blur(radius, taps_stride, batch)) return rc;
    if (log_prior == belief) return ccvpe_fail(CCVPE_EINVAL, "log_prior must not alias belief");
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    TrackPredictAffineParams p{};
    p.belief = belief; p.matrix = matrix; p.taps = taps; p.taps_stride = taps_stride; p.radius = radius; p.floor = floor;
    p.log_prior = log_prior; p.B = batch;
    launch_track_predict_affine(p, (hipStream_t)stream);
    return launch_status("track_predict_affine launch");
}

// The backward pass over stored beliefs: three launches of kernels_track_smooth.hip on the caller's stream that hand
// over through the caller's `work` - no plan, no tuning entry, nothing of the handle but its device, so calls on several streams of one
// handle do not meet.  check_smooth_args: the arguments the two smoothers share (ccvpe_track_smooth, ccvpe_track_smooth_affine), in
// the order ccvpe_track_smooth always had; motion is the shift or the matrix of the predict call.
static int check_smooth_args(ccvpe_handle h, const float* belief, const float* smoothed_next, int32_t batch, const void* motion,
                             const char* motion_name, const float* taps, int32_t taps_stride, int32_t radius, const float* floor,
                             const float* smoothed, const float* stats, const void* work) {
    if (!smoothed_next) return ccvpe_fail(CCVPE_EINVAL, "null smoothed_next");
    if (int rc = check_predict_ptrs(belief, "belief", motion, motion_name, taps, floor, smoothed, "smoothed")) return rc;
    if (!stats) return ccvpe_fail(CCVPE_EINVAL, "null stats");
    if (!work) return ccvpe_fail(CCVPE_EINVAL, "null work");
    if (int rc = check_predict_blur(radius, taps_stride, batch)) return rc;
    if (smoothed == belief || (const void*)smoothed == work || smoothed == stats) return ccvpe_fail(CCVPE_EINVAL, "smoothed must not alias belief, work or stats");
    if (stats == belief || (const void*)stats == work) return ccvpe_fail(CCVPE_EINVAL, "stats must not alias belief or work");
    if (smoothed_next == belief) return ccvpe_fail(CCVPE_EINVAL, "smoothed_next must not alias belief");
    if (((uintptr_t)belief | (uintptr_t)smoothed_next | (uintptr_t)smoothed | (uintptr_t)work) & 15)
        return ccvpe_fail(CCVPE_EINVAL, "belief, smoothed_next, smoothed and work must be 16-byte aligned");
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    return 0;
}

size_t ccvpe_track_smooth_work_bytes(int32_t batch) { return batch > 0 ? track_smooth_work_bytes(batch) : 0; }

int ccvpe_track_smooth(ccvpe_handle h, const float* belief, const float* smoothed_next, int32_t batch, const float* shift, const float* taps,
                       int32_t taps_stride, int32_t radius, const float* floor, float* smoothed, float* stats, void* work, void* stream) {
    if (int rc = check_smooth_args(h, belief, smoothed_next, batch, shift, "shift", taps, taps_stride, radius, floor, smoothed, stats, work)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    TrackSmoothParams p{};
    p.belief = belief; p.next = smoothed_next; p.shift = shift; p.taps = taps; p.taps_stride = taps_stride; p.radius = radius; p.floor = floor;
    p.smoothed = smoothed; p.stats = stats; p.work = (float*)work; p.B = batch;
    launch_track_smooth(p, (hipStream_t)stream);
    return launch_status("track_smooth launch");
}

// The same step behind ccvpe_track_predict_affine: four launches of kernels_track_smooth_affine.hip, the last one
// ccvpe_track_smooth's; ccvpe_track_smooth's checks in its order, a null matrix where a null shift stood.
size_t ccvpe_track_smooth_affine_work_bytes(int32_t batch) { return batch > 0 ? track_smooth_affine_work_bytes(batch) : 0; }

int ccvpe_track_smooth_affine(ccvpe_handle h, const float* belief, const float* smoothed_next, int32_t batch, const double* matrix,
                              const float* taps, int32_t taps_stride, int32_t radius, const float* floor, float* smoothed, float* stats,
                              void* work, void* stream) {
    if (int rc = check_smooth_args(h, belief, smoothed_next, batch, matrix, "matrix", taps, taps_stride, radius, floor, smoothed, stats, work)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    TrackSmoothAffineParams p{};
    p.belief = belief; p.next = smoothed_next; p.matrix = matrix; p.taps = taps; p.taps_stride = taps_stride; p.radius = radius; p.floor = floor;
    p.smoothed = smoothed; p.stats = stats; p.work = (float*)work; p.B = batch;
    launch_track_smooth_affine(p, (hipStream_t)stream);
    return launch_status("track_smooth_affine launch");
}

// Link statistics of a smoothed stream: four launches, the first one ccvpe_track_smooth's, on the caller's stream; like
// the smoother, nothing of the handle but its device.  Nothing is written to a map, so smoothed_next may be belief.
size_t ccvpe_track_link_work_bytes(int32_t batch, int32_t radius) {
    return batch > 0 && radius >= 0 && radius <= TRACK_MAX_R ? track_link_work_bytes(batch, radius) : 0;
}

int ccvpe_track_link(ccvpe_handle h, const float* belief, const float* smoothed_next, int32_t batch, const float* shift, const float* taps,
                     int32_t taps_stride, int32_t radius, const float* floor, float* moves, float* stats, void* work, void* stream) {
    if (!smoothed_next) return ccvpe_fail(CCVPE_EINVAL, "null smoothed_next");
    if (int rc = check_predict_ptrs(belief, "belief", shift, "shift", taps, floor, moves, "moves")) return rc;
    if (!stats) return ccvpe_fail(CCVPE_EINVAL, "null stats");
    if (!work) return ccvpe_fail(CCVPE_EINVAL, "null work");
    if (int rc = check_predict_blur(radius, taps_stride, batch)) return rc;
    const void* in[] = {belief, smoothed_next, shift, taps, floor};
    for (const void* q : in)
        if (moves == q || stats == q || work == q) return ccvpe_fail(CCVPE_EINVAL, "moves, stats and work must not alias an input");
    if (moves == stats || (const void*)moves == work || (const void*)stats == work)
        return ccvpe_fail(CCVPE_EINVAL, "moves, stats and work must not alias each other");
    if (((uintptr_t)belief | (uintptr_t)smoothed_next | (uintptr_t)work) & 15)
        return ccvpe_fail(CCVPE_EINVAL, "belief, smoothed_next and work must be 16-byte aligned");
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    TrackLinkParams p{};
    p.belief = belief; p.next = smoothed_next; p.shift = shift; p.taps = taps; p.taps_stride = taps_stride; p.radius = radius; p.floor = floor;
    p.moves = moves; p.stats = stats; p.work = (float*)work; p.B = batch;
    launch_track_link(p, (hipStream_t)stream);
    return launch_status("track_link launch");
}

// The MAP trajectory: two launches of kernels_track_viterbi.hip per frame of the forward sweep, one per backtracked
// link, on the caller's stream; like the smoother, nothing of the handle but its device.
size_t ccvpe_track_viterbi_work_bytes(int32_t batch) { return batch > 0 ? track_viterbi_work_bytes(batch) : 0; }

// check_viterbi_args: the arguments the two steps share (ccvpe_track_viterbi, ccvpe_track_viterbi_affine), in the order
// ccvpe_track_viterbi always had; motion is the shift or the matrix of the predict call.  first: the first-frame form.
static int check_viterbi_args(ccvpe_handle h, const float* belief, const float* belief_prev, const float* score_prev, const float* prev_stats,
                              int32_t batch, const void* motion, const char* motion_name, const float* taps, int32_t taps_stride,
                              int32_t radius, const float* floor, const float* score, const float* stats, const void* work, bool* first) {
    if (!belief) return ccvpe_fail(CCVPE_EINVAL, "null belief");
    const int given = (belief_prev != nullptr) + (score_prev != nullptr) + (prev_stats != nullptr) + (motion != nullptr);
    if (given != 0 && given != 4)
        return ccvpe_fail(CCVPE_EINVAL, "belief_prev, score_prev, prev_stats and %s must be all null (a stream's first frame) or all given", motion_name);
    *first = given == 0;
    if (!*first) {
        if (int rc = check_predict_ptrs(belief, "belief", motion, motion_name, taps, floor, score, "score")) return rc;
    }
    if (!score) return ccvpe_fail(CCVPE_EINVAL, "null score");
    if (!stats) return ccvpe_fail(CCVPE_EINVAL, "null stats");
    if (!work) return ccvpe_fail(CCVPE_EINVAL, "null work");
    if (!*first) {
        if (int rc = check_predict_blur(radius, taps_stride, batch)) return rc;
    }
    if (batch <= 0 || batch > PP_MAX_BATCH) return ccvpe_fail(CCVPE_EINVAL, "batch must be in 1 .. %d, got %d", PP_MAX_BATCH, batch);
    if (score == belief || score == belief_prev || score == score_prev || score == prev_stats)
        return ccvpe_fail(CCVPE_EINVAL, "score must not alias belief, belief_prev, score_prev or prev_stats");
    if ((const void*)score == work || score == stats || (const void*)stats == work) return ccvpe_fail(CCVPE_EINVAL, "score, stats and work must not alias each other");
    if (stats == belief || stats == belief_prev || stats == score_prev || stats == prev_stats)
        return ccvpe_fail(CCVPE_EINVAL, "stats must not alias belief, belief_prev, score_prev or prev_stats");
    if (((uintptr_t)belief | (uintptr_t)belief_prev | (uintptr_t)score_prev | (uintptr_t)score | (uintptr_t)work) & 15)
        return ccvpe_fail(CCVPE_EINVAL, "belief, belief_prev, score_prev, score and work must be 16-byte aligned");
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    return 0;
}
// the arguments the two backtracks share, likewise
static int check_viterbi_back_args(ccvpe_handle h, const float* score_prev, const float* prev_stats, const int32_t* cell, int32_t batch,
                                   const void* motion, const char* motion_name, const float* taps, int32_t taps_stride, int32_t radius,
                                   const float* floor, const int32_t* back) {
    if (int rc = check_predict_ptrs(score_prev, "score_prev", motion, motion_name, taps, floor, back, "back")) return rc;
    if (!prev_stats) return ccvpe_fail(CCVPE_EINVAL, "null prev_stats");
    if (!cell) return ccvpe_fail(CCVPE_EINVAL, "null cell");
    if (int rc = check_predict_blur(radius, taps_stride, batch)) return rc;
    if ((const void*)back == score_prev || (const void*)back == prev_stats || back == cell)
        return ccvpe_fail(CCVPE_EINVAL, "back must not alias score_prev, prev_stats or cell");
    if ((uintptr_t)score_prev & 15) return ccvpe_fail(CCVPE_EINVAL, "score_prev must be 16-byte aligned");
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    return 0;
}

int ccvpe_track_viterbi(ccvpe_handle h, const float* belief, const float* belief_prev, const float* score_prev, const float* prev_stats,
                        int32_t batch, const float* shift, const float* taps, int32_t taps_stride, int32_t radius, const float* floor,
                        float* score, float* stats, void* work, void* stream) {
    bool first;
    if (int rc = check_viterbi_args(h, belief, belief_prev, score_prev, prev_stats, batch, shift, "shift", taps, taps_stride, radius, floor,
                                    score, stats, work, &first)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    TrackViterbiParams p{};
    p.belief = belief; p.belief_prev = belief_prev; p.score_prev = score_prev; p.prev_stats = prev_stats; p.shift = shift;
    if (!first) { p.taps = taps; p.taps_stride = taps_stride; p.radius = radius; p.floor = floor; }
    p.score = score; p.stats = stats; p.work = (float*)work; p.B = batch;
    launch_track_viterbi(p, (hipStream_t)stream);
    return launch_status("track_viterbi launch");
}

int ccvpe_track_viterbi_back(ccvpe_handle h, const float* score_prev, const float* prev_stats, const int32_t* cell, int32_t batch,
                             const float* shift, const float* taps, int32_t taps_stride, int32_t radius, const float* floor, int32_t* back,
                             void* stream) {
    if (int rc = check_viterbi_back_args(h, score_prev, prev_stats, cell, batch, shift, "shift", taps, taps_stride, radius, floor, back)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    TrackViterbiBackParams p{};
    p.score_prev = score_prev; p.prev_stats = prev_stats; p.cell = cell; p.shift = shift; p.taps = taps; p.taps_stride = taps_stride;
    p.radius = radius; p.floor = floor; p.back = back; p.B = batch;
    launch_track_viterbi_back(p, (hipStream_t)stream);
    return launch_status("track_viterbi_back launch");
}

// The same two calls behind ccvpe_track_predict_affine: the checks of the translation entry points in their order, a
// null matrix where a null shift stood; the first-frame form is ccvpe_track_viterbi's two launches.
int ccvpe_track_viterbi_affine(ccvpe_handle h, const float* belief, const float* belief_prev, const float* score_prev,
                               const float* prev_stats, int32_t batch, const double* matrix, const float* taps, int32_t taps_stride,
                               int32_t radius, const float* floor, float* score, float* stats, void* work, void* stream) {
    bool first;
    if (int rc = check_viterbi_args(h, belief, belief_prev, score_prev, prev_stats, batch, matrix, "matrix", taps, taps_stride, radius, floor,
                                    score, stats, work, &first)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    TrackViterbiAffineParams p{};
    p.belief = belief; p.belief_prev = belief_prev; p.score_prev = score_prev; p.prev_stats = prev_stats; p.matrix = matrix;
    if (!first) { p.taps = taps; p.taps_stride = taps_stride; p.radius = radius; p.floor = floor; }
    p.score = score; p.stats = stats; p.work = (float*)work; p.B = batch;
    launch_track_viterbi_affine(p, (hipStream_t)stream);
    return launch_status("track_viterbi_affine launch");
}

int ccvpe_track_viterbi_back_affine(ccvpe_handle h, const float* score_prev, const float* prev_stats, const int32_t* cell, int32_t batch,
                                    const double* matrix, const float* taps, int32_t taps_stride, int32_t radius, const float* floor,
                                    int32_t* back, void* stream) {
    if (int rc = check_viterbi_back_args(h, score_prev, prev_stats, cell, batch, matrix, "matrix", taps, taps_stride, radius, floor, back)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    TrackViterbiBackAffineParams p{};
    p.score_prev = score_prev; p.prev_stats = prev_stats; p.cell = cell; p.matrix = matrix; p.taps = taps; p.taps_stride = taps_stride;
    p.radius = radius; p.floor = floor; p.back = back; p.B = batch;
    launch_track_viterbi_back_affine(p, (hipStream_t)stream);
    return launch_status("track_viterbi_back_affine launch");
}

// ------------------------------------------------------------------------------------------------
// Posterior summary: the argmax pose plans with the summary row as one more output of pose.argmax (plans of their own,
// PlanKey::summary, for the float64 hand-off in the workspace; the launches, names and tuning entries of the pose plans), the logits
// form on the prior scratch, and one launch of belief_summary_kernel for a stored map.
// ------------------------------------------------------------------------------------------------
// log_prior and posterior may be null; the posterior's aliasing rules are ccvpe_track_update's
static int check_summary_args(const float* log_prior, int64_t prior_stride, int32_t radius, const float* rows, const float* summary,
                              const float* posterior) {
    if (!rows) return ccvpe_fail(CCVPE_EINVAL, "null rows");
    if (!summary) return ccvpe_fail(CCVPE_EINVAL, "null summary");
    if (radius < 0 || radius > SUMMARY_MAX_R) return ccvpe_fail(CCVPE_EINVAL, "radius must be in 0 .. %d, got %d", SUMMARY_MAX_R, radius);
    if (log_prior) if (int rc = check_prior_stride(prior_stride)) return rc;
    if (summary == rows) return ccvpe_fail(CCVPE_EINVAL, "summary must not alias rows");
    if (posterior && log_prior && (const float*)log_prior == posterior) return ccvpe_fail(CCVPE_EINVAL, "posterior must not alias log_prior");
    if (posterior && (posterior == summary || posterior == rows)) return ccvpe_fail(CCVPE_EINVAL, "posterior must not alias rows or summary");
    return 0;
}

int ccvpe_localize_summary(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const float* sat, int32_t batch,
                           const float* log_prior, int64_t prior_stride, int32_t radius, float* rows, float* summary, float* posterior,
                           void* stream) {
    if (!grd) return ccvpe_fail(CCVPE_EINVAL, "null grd");
    if (!sat) return ccvpe_fail(CCVPE_EINVAL, "null sat");
    if (int rc = check_summary_args(log_prior, prior_stride, radius, rows, summary, posterior)) return rc;
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.sat = sat; fc.tail.rows = rows; fc.tail.log_prior = log_prior; fc.tail.prior_stride = log_prior ? prior_stride : 0; fc.tail.posterior = posterior;
    fc.tail.summary = summary; fc.tail.summary_r = radius;
    return run_forward(h, fc);
}

int ccvpe_localize_summary_cached_indexed(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache, int32_t n_tiles,
                                          const int32_t* tile_index, int32_t batch, const float* log_prior, int64_t prior_stride,
                                          int32_t radius, float* rows, float* summary, float* posterior, void* stream) {
    if (int rc = check_cached_args(grd, cache, n_tiles, tile_index, batch, rows)) return rc;
    if (int rc = check_summary_args(log_prior, prior_stride, radius, rows, summary, posterior)) return rc;
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.cache = (const float*)cache; fc.tile_index = tile_index; fc.n_tiles = n_tiles;
    fc.tail.rows = rows; fc.tail.log_prior = log_prior; fc.tail.prior_stride = log_prior ? prior_stride : 0; fc.tail.posterior = posterior;
    fc.tail.summary = summary; fc.tail.summary_r = radius;
    return run_forward(h, fc);
}

int ccvpe_postprocess_summary(ccvpe_handle h, const float* logits, const float* ori, int32_t batch, const float* log_prior,
                              int64_t prior_stride, int32_t radius, float* rows, float* summary, float* posterior, void* stream) {
    if (!logits) return ccvpe_fail(CCVPE_EINVAL, "null logits");
    if (!ori) return ccvpe_fail(CCVPE_EINVAL, "null ori");
    if (int rc = check_summary_args(log_prior, prior_stride, radius, rows, summary, posterior)) return rc;
    if (posterior && posterior == logits) return ccvpe_fail(CCVPE_EINVAL, "posterior must not alias logits");
    if (batch <= 0 || batch > PP_MAX_BATCH) return ccvpe_fail(CCVPE_EINVAL, "batch must be in 1 .. %d, got %d", PP_MAX_BATCH, batch);
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    TailCall t;
    t.rows = rows; t.log_prior = log_prior; t.prior_stride = log_prior ? prior_stride : 0; t.posterior = posterior;
    t.summary = summary; t.summary_r = radius;
    if (int rc = run_logits_tail(h, logits, ori, batch, t, (hipStream_t)stream)) return rc;
    return launch_status("postprocess_summary launch");
}

int ccvpe_belief_summary(ccvpe_handle h, const float* belief, int32_t batch, int32_t radius, float* summary, void* stream) {
    if (!belief) return ccvpe_fail(CCVPE_EINVAL, "null belief");
    if (!summary) return ccvpe_fail(CCVPE_EINVAL, "null summary");
    if (radius < 0 || radius > SUMMARY_MAX_R) return ccvpe_fail(CCVPE_EINVAL, "radius must be in 0 .. %d, got %d", SUMMARY_MAX_R, radius);
    if (batch <= 0 || batch > PP_MAX_BATCH) return ccvpe_fail(CCVPE_EINVAL, "batch must be in 1 .. %d, got %d", PP_MAX_BATCH, batch);
    if (summary == belief) return ccvpe_fail(CCVPE_EINVAL, "summary must not alias belief");
    if (((uintptr_t)belief & 3) != 0) return ccvpe_fail(CCVPE_EINVAL, "belief must be 4-byte aligned");
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    if (int rc = ensure_scratch(h->prior_scratch, batch, prior_scratch_bytes, "prior post-processing scratch")) return rc;
    const TailBuffers w = scratch_buffers(h->prior_scratch, nullptr, nullptr);
    BeliefSummaryParams p{};
    p.belief = belief; p.B = batch; p.r = radius; p.pairs = reinterpret_cast<float*>(w.keys); p.summ_part = w.summ_part; p.tickets = w.tickets;
    p.summary = summary;
    launch_belief_summary(p, (hipStream_t)stream);
    return launch_status("belief_summary launch");
}

// ------------------------------------------------------------------------------------------------
// Heading posterior: the argmax pose plans with the whole orientation field in the workspace and one more launch,
// pose.heading, behind both decoders (plans of their own, PlanKey::heading; every other launch keeps the name and tuning entry it has
// in the pose or the full plan), and the logits form on the prior scratch.  summary and posterior are optional outputs of pose.argmax
// as in the summary forms.
// ------------------------------------------------------------------------------------------------
static int check_heading_args(const float* log_prior, int64_t prior_stride, int32_t radius, int32_t nbins, const float* rows,
                              const float* heading, const float* hist, const float* summary, const float* posterior) {
    if (!rows) return ccvpe_fail(CCVPE_EINVAL, "null rows");
    if (!heading) return ccvpe_fail(CCVPE_EINVAL, "null heading");
    if (!hist) return ccvpe_fail(CCVPE_EINVAL, "null hist");
    if (nbins < HEADING_MIN_BINS || nbins > HEADING_MAX_BINS)
        return ccvpe_fail(CCVPE_EINVAL, "nbins must be in %d .. %d, got %d", HEADING_MIN_BINS, HEADING_MAX_BINS, nbins);
    if (radius < 0 || radius > HEADING_MAX_R) return ccvpe_fail(CCVPE_EINVAL, "radius must be in 0 .. %d, got %d", HEADING_MAX_R, radius);
    if (log_prior) if (int rc = check_prior_stride(prior_stride)) return rc;
    if (heading == rows || hist == rows || heading == hist) return ccvpe_fail(CCVPE_EINVAL, "rows, heading and hist must not alias");
    if (log_prior && (heading == log_prior || hist == log_prior)) return ccvpe_fail(CCVPE_EINVAL, "heading and hist must not alias log_prior");
    if (summary && (summary == rows || summary == heading || summary == hist))
        return ccvpe_fail(CCVPE_EINVAL, "summary must not alias rows, heading or hist");
    if (posterior && log_prior && (const float*)log_prior == posterior) return ccvpe_fail(CCVPE_EINVAL, "posterior must not alias log_prior");
    if (posterior && (posterior == rows || posterior == summary || posterior == heading || posterior == hist))
        return ccvpe_fail(CCVPE_EINVAL, "posterior must not alias rows, summary, heading or hist");
    return 0;
}

static TailCall heading_call(const float* log_prior, int64_t prior_stride, int32_t radius, int32_t nbins, float* rows, float* heading,
                             float* hist, float* summary, float* posterior) {
    TailCall t;
    t.rows = rows; t.log_prior = log_prior; t.prior_stride = log_prior ? prior_stride : 0; t.posterior = posterior;
    t.summary = summary; t.summary_r = radius;
    t.heading = heading; t.hist = hist; t.heading_bins = nbins; t.heading_r = radius;
    return t;
}

int ccvpe_localize_heading(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const float* sat, int32_t batch,
                           const float* log_prior, int64_t prior_stride, int32_t radius, int32_t nbins, float* rows, float* heading,
                           float* hist, float* summary, float* posterior, void* stream) {
    if (!grd) return ccvpe_fail(CCVPE_EINVAL, "null grd");
    if (!sat) return ccvpe_fail(CCVPE_EINVAL, "null sat");
    if (int rc = check_heading_args(log_prior, prior_stride, radius, nbins, rows, heading, hist, summary, posterior)) return rc;
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.sat = sat;
    fc.tail = heading_call(log_prior, prior_stride, radius, nbins, rows, heading, hist, summary, posterior);
    return run_forward(h, fc);
}

int ccvpe_localize_heading_cached_indexed(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache, int32_t n_tiles,
                                          const int32_t* tile_index, int32_t batch, const float* log_prior, int64_t prior_stride,
                                          int32_t radius, int32_t nbins, float* rows, float* heading, float* hist, float* summary,
                                          float* posterior, void* stream) {
    if (int rc = check_cached_args(grd, cache, n_tiles, tile_index, batch, rows)) return rc;
    if (int rc = check_heading_args(log_prior, prior_stride, radius, nbins, rows, heading, hist, summary, posterior)) return rc;
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.cache = (const float*)cache; fc.tile_index = tile_index; fc.n_tiles = n_tiles;
    fc.tail = heading_call(log_prior, prior_stride, radius, nbins, rows, heading, hist, summary, posterior);
    return run_forward(h, fc);
}

int ccvpe_postprocess_heading(ccvpe_handle h, const float* logits, const float* ori, int32_t batch, const float* log_prior,
                              int64_t prior_stride, int32_t radius, int32_t nbins, float* rows, float* heading, float* hist, float* summary,
                              float* posterior, void* stream) {
    if (!logits) return ccvpe_fail(CCVPE_EINVAL, "null logits");
    if (!ori) return ccvpe_fail(CCVPE_EINVAL, "null ori");
    if (int rc = check_heading_args(log_prior, prior_stride, radius, nbins, rows, heading, hist, summary, posterior)) return rc;
    if (posterior && posterior == logits) return ccvpe_fail(CCVPE_EINVAL, "posterior must not alias logits");
    if (heading == logits || heading == ori || hist == logits || hist == ori)
        return ccvpe_fail(CCVPE_EINVAL, "heading and hist must not alias logits or ori");
    if (batch <= 0 || batch > PP_MAX_BATCH) return ccvpe_fail(CCVPE_EINVAL, "batch must be in 1 .. %d, got %d", PP_MAX_BATCH, batch);
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    const TailCall t = heading_call(log_prior, prior_stride, radius, nbins, rows, heading, hist, summary, posterior);
    if (int rc = run_logits_tail(h, logits, ori, batch, t, (hipStream_t)stream)) return rc;
    return launch_status("postprocess_heading launch");
}

// ------------------------------------------------------------------------------------------------
// Heading prior: a table of nb + 1 log-weights per query, read through the orientation field into a combined prior map
// (heading_prior_map_kernel) that every prior form takes as its log_prior.  The network forms run the heading plans with that map in
// the workspace (PlanKey::hprior: one launch more, pose.hprior, and the tail behind the orientation decoder); ccvpe_heading_prior_map
// is the launch alone on forward outputs the caller holds; ccvpe_heading_predict turns a hist into the next frame's table.
// ------------------------------------------------------------------------------------------------
static int check_hprior_table(const float* table, int32_t table_stride, int32_t nb) {
    if (!table) return ccvpe_fail(CCVPE_EINVAL, "null table");
    if (nb < HEADING_MIN_BINS || nb > HEADING_MAX_BINS)
        return ccvpe_fail(CCVPE_EINVAL, "nb must be in %d .. %d, got %d", HEADING_MIN_BINS, HEADING_MAX_BINS, nb);
    if (table_stride != 0 && table_stride != nb + 1)
        return ccvpe_fail(CCVPE_EINVAL, "table_stride must be 0 (one table) or nb + 1 = %d (one per query), got %d", nb + 1, table_stride);
    return 0;
}

int ccvpe_heading_prior_map(ccvpe_handle h, const float* ori, int32_t batch, const float* log_prior, int64_t prior_stride,
                            const float* table, int32_t table_stride, int32_t nb, float* out_map, void* stream) {
    if (!ori) return ccvpe_fail(CCVPE_EINVAL, "null ori");
    if (!out_map) return ccvpe_fail(CCVPE_EINVAL, "null out_map");
    if (int rc = check_hprior_table(table, table_stride, nb)) return rc;
    if (log_prior) if (int rc = check_prior_stride(prior_stride)) return rc;
    if (batch <= 0 || batch > PP_MAX_BATCH) return ccvpe_fail(CCVPE_EINVAL, "batch must be in 1 .. %d, got %d", PP_MAX_BATCH, batch);
    if (out_map == ori) return ccvpe_fail(CCVPE_EINVAL, "out_map must not alias ori");
    if (log_prior && out_map == log_prior) return ccvpe_fail(CCVPE_EINVAL, "out_map must not alias log_prior");
    if (out_map == table) return ccvpe_fail(CCVPE_EINVAL, "out_map must not alias table");
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    HeadingPriorMapParams p{};
    p.ori = ori; p.prior = log_prior; p.prior_stride = log_prior ? prior_stride : 0; p.table = table; p.table_stride = table_stride; p.nb = nb;
    p.out = out_map; p.B = batch;
    launch_heading_prior_map(p, (hipStream_t)stream);
    return launch_status("heading_prior_map launch");
}

// the heading prior's own arguments, then the checks of the matching heading form
static int check_heading_prior_args(const float* table, int32_t table_stride, int32_t nb, const float* log_prior, int64_t prior_stride,
                                    int32_t radius, int32_t nbins, const float* rows, const float* heading, const float* hist,
                                    const float* summary, const float* posterior) {
    if (int rc = check_hprior_table(table, table_stride, nb)) return rc;
    if (int rc = check_heading_args(log_prior, prior_stride, radius, nbins, rows, heading, hist, summary, posterior)) return rc;
    if (table == rows || table == heading || table == hist || (summary && table == summary) || (posterior && table == posterior))
        return ccvpe_fail(CCVPE_EINVAL, "table must not alias rows, heading, hist, summary or posterior");
    return 0;
}

int ccvpe_localize_heading_prior(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const float* sat, int32_t batch,
                                 const float* log_prior, int64_t prior_stride, const float* table, int32_t table_stride, int32_t nb,
                                 int32_t radius, int32_t nbins, float* rows, float* heading, float* hist, float* summary, float* posterior,
                                 void* stream) {
    if (!grd) return ccvpe_fail(CCVPE_EINVAL, "null grd");
    if (!sat) return ccvpe_fail(CCVPE_EINVAL, "null sat");
    if (int rc = check_heading_prior_args(table, table_stride, nb, log_prior, prior_stride, radius, nbins, rows, heading, hist, summary, posterior))
        return rc;
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.sat = sat;
    fc.tail = heading_call(log_prior, prior_stride, radius, nbins, rows, heading, hist, summary, posterior);
    fc.tail.hprior_table = table; fc.tail.hprior_stride = table_stride; fc.tail.hprior_nb = nb;
    return run_forward(h, fc);
}

int ccvpe_localize_heading_prior_cached_indexed(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache,
                                                int32_t n_tiles, const int32_t* tile_index, int32_t batch, const float* log_prior,
                                                int64_t prior_stride, const float* table, int32_t table_stride, int32_t nb, int32_t radius,
                                                int32_t nbins, float* rows, float* heading, float* hist, float* summary, float* posterior,
                                                void* stream) {
    if (int rc = check_cached_args(grd, cache, n_tiles, tile_index, batch, rows)) return rc;
    if (int rc = check_heading_prior_args(table, table_stride, nb, log_prior, prior_stride, radius, nbins, rows, heading, hist, summary, posterior))
        return rc;
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.cache = (const float*)cache; fc.tile_index = tile_index; fc.n_tiles = n_tiles;
    fc.tail = heading_call(log_prior, prior_stride, radius, nbins, rows, heading, hist, summary, posterior);
    fc.tail.hprior_table = table; fc.tail.hprior_stride = table_stride; fc.tail.hprior_nb = nb;
    return run_forward(h, fc);
}

int ccvpe_heading_predict(ccvpe_handle h, const float* hist, int32_t batch, int32_t nb, const float* turn_deg, const float* taps,
                          int32_t taps_stride, int32_t radius, const float* floor, float* out, void* stream) {
    if (int rc = check_predict_ptrs(hist, "hist", turn_deg, "turn_deg", taps, floor, out, "out")) return rc;
    if (nb < HEADING_MIN_BINS || nb > HEADING_MAX_BINS)
        return ccvpe_fail(CCVPE_EINVAL, "nb must be in %d .. %d, got %d", HEADING_MIN_BINS, HEADING_MAX_BINS, nb);
    if (int rc = check_predict_blur(radius, taps_stride, batch, nb)) return rc;
    if (out == hist) return ccvpe_fail(CCVPE_EINVAL, "out must not alias hist");
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    HeadingPredictParams p{};
    p.hist = hist; p.turn_deg = turn_deg; p.taps = taps; p.taps_stride = taps_stride; p.radius = radius; p.floor = floor; p.out = out;
    p.B = batch; p.nb = nb;
    launch_heading_predict(p, (hipStream_t)stream);
    return launch_status("heading_predict launch");
}

// ------------------------------------------------------------------------------------------------
// Joint position-heading filter: a histogram filter over (heading bin, cell), kernels_track_joint.hip.  Predict: two
// launches on the caller's stream that hand over through the caller's `work`; nothing of the handle but its device.  Update: four
// launches over forward outputs the caller holds, through the handle's joint scratch.  No plan, no tuning entry.
// ------------------------------------------------------------------------------------------------
static int check_joint_shape(int32_t batch, int32_t nb) {
    if (nb < JOINT_MIN_BINS || nb > JOINT_MAX_BINS) return ccvpe_fail(CCVPE_EINVAL, "nb must be in %d .. %d, got %d", JOINT_MIN_BINS, JOINT_MAX_BINS, nb);
    if (batch <= 0 || (int64_t)batch * nb > JOINT_MAX_SLICES)
        return ccvpe_fail(CCVPE_EINVAL, "batch must be >= 1 with batch * nb <= %d, got batch %d, nb %d", JOINT_MAX_SLICES, batch, nb);
    return 0;
}

size_t ccvpe_track_joint_work_bytes(int32_t batch, int32_t nb) {
    return batch > 0 && nb >= JOINT_MIN_BINS && nb <= JOINT_MAX_BINS && (int64_t)batch * nb <= JOINT_MAX_SLICES ? track_joint_work_bytes(batch, nb) : 0;
}

int ccvpe_track_joint_predict(ccvpe_handle h, const float* joint, int32_t batch, int32_t nb, const float* shift, const float* taps,
                              int32_t taps_stride, int32_t radius, const float* turn_deg, const float* htaps, int32_t htaps_stride,
                              int32_t hradius, const float* floor, void* work, float* prior, void* stream) {
    if (int rc = check_predict_ptrs(joint, "joint", shift, "shift", taps, floor, prior, "prior")) return rc;
    if (!turn_deg) return ccvpe_fail(CCVPE_EINVAL, "null turn_deg");
    if (!htaps) return ccvpe_fail(CCVPE_EINVAL, "null htaps");
    if (!work) return ccvpe_fail(CCVPE_EINVAL, "null work");
    if (int rc = check_joint_shape(batch, nb)) return rc;
    if (int rc = check_predict_blur(radius, taps_stride, batch)) return rc;
    if (hradius < 0 || hradius > TRACK_MAX_R || 2 * hradius + 1 > nb)
        return ccvpe_fail(CCVPE_EINVAL, "hradius must be in 0 .. %d with 2 hradius + 1 <= nb = %d, got %d", TRACK_MAX_R, nb, hradius);
    if (htaps_stride != 0 && htaps_stride != hradius + 1)
        return ccvpe_fail(CCVPE_EINVAL, "htaps_stride must be 0 (one set of taps) or hradius + 1 = %d (one per query), got %d", hradius + 1,
                          htaps_stride);
    if (prior == joint || (const void*)prior == work || (const void*)joint == work)
        return ccvpe_fail(CCVPE_EINVAL, "joint, work and prior must not alias each other");
    if (((uintptr_t)joint | (uintptr_t)work | (uintptr_t)prior) & 15) return ccvpe_fail(CCVPE_EINVAL, "joint, work and prior must be 16-byte aligned");
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    TrackJointPredictParams p{};
    p.joint = joint; p.shift = shift; p.taps = taps; p.taps_stride = taps_stride; p.radius = radius; p.turn_deg = turn_deg; p.htaps = htaps;
    p.htaps_stride = htaps_stride; p.hradius = hradius; p.floor = floor; p.work = (float*)work; p.prior = prior; p.B = batch; p.nb = nb;
    launch_track_joint_predict(p, (hipStream_t)stream);
    return launch_status("track_joint_predict launch");
}

// The same step under an affine map per source heading bin: the checks of ccvpe_track_joint_predict in their order, the
// matrix in the shift's place; always the affine kernel, as ccvpe_track_predict_affine.
int ccvpe_track_joint_predict_affine(ccvpe_handle h, const float* joint, int32_t batch, int32_t nb, const double* matrix, const float* taps,
                                     int32_t taps_stride, int32_t radius, const float* turn_deg, const float* htaps, int32_t htaps_stride,
                                     int32_t hradius, const float* floor, void* work, float* prior, void* stream) {
    if (int rc = check_predict_ptrs(joint, "joint", matrix, "matrix", taps, floor, prior, "prior")) return rc;
    if (!turn_deg) return ccvpe_fail(CCVPE_EINVAL, "null turn_deg");
    if (!htaps) return ccvpe_fail(CCVPE_EINVAL, "null htaps");
    if (!work) return ccvpe_fail(CCVPE_EINVAL, "null work");
    if (int rc = check_joint_shape(batch, nb)) return rc;
    if (int rc = check_predict_blur(radius, taps_stride, batch)) return rc;
    if (hradius < 0 || hradius > TRACK_MAX_R || 2 * hradius + 1 > nb)
        return ccvpe_fail(CCVPE_EINVAL, "hradius must be in 0 .. %d with 2 hradius + 1 <= nb = %d, got %d", TRACK_MAX_R, nb, hradius);
    if (htaps_stride != 0 && htaps_stride != hradius + 1)
        return ccvpe_fail(CCVPE_EINVAL, "htaps_stride must be 0 (one set of taps) or hradius + 1 = %d (one per query), got %d", hradius + 1,
                          htaps_stride);
    if (prior == joint || (const void*)prior == work || (const void*)joint == work)
        return ccvpe_fail(CCVPE_EINVAL, "joint, work and prior must not alias each other");
    if (((uintptr_t)joint | (uintptr_t)work | (uintptr_t)prior) & 15) return ccvpe_fail(CCVPE_EINVAL, "joint, work and prior must be 16-byte aligned");
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    TrackJointPredictAffineParams p{};
    p.joint = joint; p.matrix = matrix; p.taps = taps; p.taps_stride = taps_stride; p.radius = radius; p.turn_deg = turn_deg; p.htaps = htaps;
    p.htaps_stride = htaps_stride; p.hradius = hradius; p.floor = floor; p.work = (float*)work; p.prior = prior; p.B = batch; p.nb = nb;
    launch_track_joint_predict_affine(p, (hipStream_t)stream);
    return launch_status("track_joint_predict_affine launch");
}

int ccvpe_track_joint_update_logits(ccvpe_handle h, const float* logits, const float* ori, int32_t batch, const float* prior,
                                    const float* emission, int32_t emission_stride, int32_t nb, float* rows, float* joint_out,
                                    float* marginal, float* hist, void* stream) {
    if (!logits) return ccvpe_fail(CCVPE_EINVAL, "null logits");
    if (!ori) return ccvpe_fail(CCVPE_EINVAL, "null ori");
    if (!emission) return ccvpe_fail(CCVPE_EINVAL, "null emission");
    if (!rows) return ccvpe_fail(CCVPE_EINVAL, "null rows");
    if (!joint_out) return ccvpe_fail(CCVPE_EINVAL, "null joint_out");
    if (!marginal) return ccvpe_fail(CCVPE_EINVAL, "null marginal");
    if (!hist) return ccvpe_fail(CCVPE_EINVAL, "null hist");
    if (int rc = check_joint_shape(batch, nb)) return rc;
    if (emission_stride != 0 && emission_stride != nb + 1)
        return ccvpe_fail(CCVPE_EINVAL, "emission_stride must be 0 (one table) or nb + 1 = %d (one per query), got %d", nb + 1, emission_stride);
    const void* in[] = {logits, ori, emission};
    const void* out[] = {rows, joint_out, marginal, hist};
    for (const void* o : out) {
        for (const void* q : in)
            if (o == q) return ccvpe_fail(CCVPE_EINVAL, "rows, joint_out, marginal and hist must not alias logits, ori or emission");
        if (o != joint_out && o == prior) return ccvpe_fail(CCVPE_EINVAL, "rows, marginal and hist must not alias prior");
    }
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (out[i] == out[j]) return ccvpe_fail(CCVPE_EINVAL, "rows, joint_out, marginal and hist must not alias each other");
    if (((uintptr_t)logits | (uintptr_t)ori | (uintptr_t)prior | (uintptr_t)joint_out | (uintptr_t)marginal) & 15)
        return ccvpe_fail(CCVPE_EINVAL, "logits, ori, prior, joint_out and marginal must be 16-byte aligned");
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    if (int rc = ensure_scratch(h->joint_scratch, batch, track_joint_scratch_bytes, "joint filter scratch")) return rc;
    TrackJointUpdateParams p{};
    p.logits = logits; p.ori = ori; p.prior = prior; p.emission = emission; p.emission_stride = emission_stride; p.rows = rows;
    p.joint_out = joint_out; p.marginal = marginal; p.hist = hist; p.B = batch; p.nb = nb;
    track_joint_scratch(h->joint_scratch.ptr, h->joint_scratch.batch, p);
    launch_track_joint_update(p, (hipStream_t)stream);
    return launch_status("track_joint_update_logits launch");
}

// The backward step of the joint filter: five launches of kernels_track_joint.hip's first kernel and
// kernels_track_joint_smooth.hip on the caller's stream that hand over through the caller's `work` - nothing of the handle but its
// device, so calls on several streams of one handle do not meet.
size_t ccvpe_track_joint_smooth_work_bytes(int32_t batch, int32_t nb) {
    return batch > 0 && nb >= JOINT_MIN_BINS && nb <= JOINT_MAX_BINS && (int64_t)batch * nb <= JOINT_MAX_SLICES ? track_joint_smooth_work_bytes(batch, nb) : 0;
}

int ccvpe_track_joint_smooth(ccvpe_handle h, const float* joint, const float* smoothed_next, int32_t batch, int32_t nb, const float* shift,
                             const float* taps, int32_t taps_stride, int32_t radius, const float* turn_deg, const float* htaps,
                             int32_t htaps_stride, int32_t hradius, const float* floor, void* work, float* smoothed, float* marginal,
                             float* hist, float* stats, void* stream) {
    if (int rc = check_predict_ptrs(joint, "joint", shift, "shift", taps, floor, smoothed, "smoothed")) return rc;
    if (!smoothed_next) return ccvpe_fail(CCVPE_EINVAL, "null smoothed_next");
    if (!turn_deg) return ccvpe_fail(CCVPE_EINVAL, "null turn_deg");
    if (!htaps) return ccvpe_fail(CCVPE_EINVAL, "null htaps");
    if (!work) return ccvpe_fail(CCVPE_EINVAL, "null work");
    if (!marginal) return ccvpe_fail(CCVPE_EINVAL, "null marginal");
    if (!hist) return ccvpe_fail(CCVPE_EINVAL, "null hist");
    if (!stats) return ccvpe_fail(CCVPE_EINVAL, "null stats");
    if (int rc = check_joint_shape(batch, nb)) return rc;
    if (int rc = check_predict_blur(radius, taps_stride, batch)) return rc;
    if (hradius < 0 || hradius > TRACK_MAX_R || 2 * hradius + 1 > nb)
        return ccvpe_fail(CCVPE_EINVAL, "hradius must be in 0 .. %d with 2 hradius + 1 <= nb = %d, got %d", TRACK_MAX_R, nb, hradius);
    if (htaps_stride != 0 && htaps_stride != hradius + 1)
        return ccvpe_fail(CCVPE_EINVAL, "htaps_stride must be 0 (one set of taps) or hradius + 1 = %d (one per query), got %d", hradius + 1,
                          htaps_stride);
    const void* in[] = {joint, smoothed_next, shift, taps, turn_deg, htaps, floor, work};
    const void* out[] = {smoothed, marginal, hist, stats};
    for (const void* o : out)
        for (const void* q : in)
            if (o == q && !(o == smoothed && q == smoothed_next))
                return ccvpe_fail(CCVPE_EINVAL, "smoothed, marginal, hist and stats must not alias an input or work (smoothed == smoothed_next excepted)");
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (out[i] == out[j]) return ccvpe_fail(CCVPE_EINVAL, "smoothed, marginal, hist and stats must not alias each other");
    if (smoothed_next == joint || (const void*)joint == work || (const void*)smoothed_next == work)
        return ccvpe_fail(CCVPE_EINVAL, "joint, smoothed_next and work must not alias each other");
    if (((uintptr_t)joint | (uintptr_t)smoothed_next | (uintptr_t)work | (uintptr_t)smoothed | (uintptr_t)marginal) & 15)
        return ccvpe_fail(CCVPE_EINVAL, "joint, smoothed_next, work, smoothed and marginal must be 16-byte aligned");
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    TrackJointSmoothParams p{};
    p.joint = joint; p.next = smoothed_next; p.shift = shift; p.taps = taps; p.taps_stride = taps_stride; p.radius = radius;
    p.turn_deg = turn_deg; p.htaps = htaps; p.htaps_stride = htaps_stride; p.hradius = hradius; p.floor = floor; p.work = (float*)work;
    p.smoothed = smoothed; p.marginal = marginal; p.hist = hist; p.stats = stats; p.B = batch; p.nb = nb;
    launch_track_joint_smooth(p, (hipStream_t)stream);
    return launch_status("track_joint_smooth launch");
}

// The MAP trajectory of a joint stream: four launches of kernels_track_joint.hip's first kernel and
// kernels_track_joint_viterbi.hip per frame of the forward sweep (two for a stream's first frame), one per backtracked link, on the
// caller's stream; the refusals are the joint smoother's, and like it nothing of the handle is used but its device.
size_t ccvpe_track_joint_viterbi_work_bytes(int32_t batch, int32_t nb) {
    return batch > 0 && nb >= JOINT_MIN_BINS && nb <= JOINT_MAX_BINS && (int64_t)batch * nb <= JOINT_MAX_SLICES ? track_joint_viterbi_work_bytes(batch, nb) : 0;
}

// the ranges the step and the link share behind their pointer checks
static int check_joint_viterbi_motion(int32_t batch, int32_t nb, int32_t taps_stride, int32_t radius, int32_t htaps_stride, int32_t hradius) {
    if (int rc = check_predict_blur(radius, taps_stride, batch)) return rc;
    if (hradius < 0 || hradius > TRACK_MAX_R || 2 * hradius + 1 > nb)
        return ccvpe_fail(CCVPE_EINVAL, "hradius must be in 0 .. %d with 2 hradius + 1 <= nb = %d, got %d", TRACK_MAX_R, nb, hradius);
    if (htaps_stride != 0 && htaps_stride != hradius + 1)
        return ccvpe_fail(CCVPE_EINVAL, "htaps_stride must be 0 (one set of taps) or hradius + 1 = %d (one per query), got %d", hradius + 1,
                          htaps_stride);
    return 0;
}

int ccvpe_track_joint_viterbi(ccvpe_handle h, const float* joint, const float* joint_prev, const float* score_prev, const float* prev_stats,
                              int32_t batch, int32_t nb, const float* shift, const float* taps, int32_t taps_stride, int32_t radius,
                              const float* turn_deg, const float* htaps, int32_t htaps_stride, int32_t hradius, const float* floor,
                              void* work, float* score, float* stats, void* stream) {
    if (!joint) return ccvpe_fail(CCVPE_EINVAL, "null joint");
    const int given = (joint_prev != nullptr) + (score_prev != nullptr) + (prev_stats != nullptr) + (shift != nullptr);
    if (given != 0 && given != 4)
        return ccvpe_fail(CCVPE_EINVAL, "joint_prev, score_prev, prev_stats and shift must be all null (a stream's first frame) or all given");
    const bool first = given == 0;
    if (!first) {
        if (int rc = check_predict_ptrs(joint, "joint", shift, "shift", taps, floor, score, "score")) return rc;
        if (!turn_deg) return ccvpe_fail(CCVPE_EINVAL, "null turn_deg");
        if (!htaps) return ccvpe_fail(CCVPE_EINVAL, "null htaps");
    }
    if (!work) return ccvpe_fail(CCVPE_EINVAL, "null work");
    if (!score) return ccvpe_fail(CCVPE_EINVAL, "null score");
    if (!stats) return ccvpe_fail(CCVPE_EINVAL, "null stats");
    if (int rc = check_joint_shape(batch, nb)) return rc;
    if (!first) {
        if (int rc = check_joint_viterbi_motion(batch, nb, taps_stride, radius, htaps_stride, hradius)) return rc;
    }
    const void* in[] = {joint, joint_prev, score_prev, prev_stats, shift, taps, turn_deg, htaps, floor, work};
    for (const void* q : in)
        if (q && (q == (const void*)score || q == (const void*)stats))
            return ccvpe_fail(CCVPE_EINVAL, "score and stats must not alias an input or work");
    if (score == stats) return ccvpe_fail(CCVPE_EINVAL, "score and stats must not alias each other");
    if ((const void*)joint == work || (joint_prev && (const void*)joint_prev == work) || (score_prev && (const void*)score_prev == work))
        return ccvpe_fail(CCVPE_EINVAL, "joint, joint_prev, score_prev and work must not alias each other");
    if (((uintptr_t)joint | (uintptr_t)joint_prev | (uintptr_t)score_prev | (uintptr_t)work | (uintptr_t)score) & 15)
        return ccvpe_fail(CCVPE_EINVAL, "joint, joint_prev, score_prev, work and score must be 16-byte aligned");
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    TrackJointViterbiParams p{};
    p.joint = joint; p.joint_prev = joint_prev; p.score_prev = score_prev; p.prev_stats = prev_stats; p.shift = shift;
    if (!first) {
        p.taps = taps; p.taps_stride = taps_stride; p.radius = radius; p.turn_deg = turn_deg; p.htaps = htaps; p.htaps_stride = htaps_stride;
        p.hradius = hradius; p.floor = floor;
    }
    p.work = (float*)work; p.score = score; p.stats = stats; p.B = batch; p.nb = nb;
    launch_track_joint_viterbi(p, (hipStream_t)stream);
    return launch_status("track_joint_viterbi launch");
}

int ccvpe_track_joint_viterbi_back(ccvpe_handle h, const float* score_prev, const float* prev_stats, const int32_t* cell, const int32_t* bin,
                                   int32_t batch, int32_t nb, const float* shift, const float* taps, int32_t taps_stride, int32_t radius,
                                   const float* turn_deg, const float* htaps, int32_t htaps_stride, int32_t hradius, const float* floor,
                                   int32_t* back, void* stream) {
    if (int rc = check_predict_ptrs(score_prev, "score_prev", shift, "shift", taps, floor, back, "back")) return rc;
    if (!prev_stats) return ccvpe_fail(CCVPE_EINVAL, "null prev_stats");
    if (!cell) return ccvpe_fail(CCVPE_EINVAL, "null cell");
    if (!bin) return ccvpe_fail(CCVPE_EINVAL, "null bin");
    if (!turn_deg) return ccvpe_fail(CCVPE_EINVAL, "null turn_deg");
    if (!htaps) return ccvpe_fail(CCVPE_EINVAL, "null htaps");
    if (int rc = check_joint_shape(batch, nb)) return rc;
    if (int rc = check_joint_viterbi_motion(batch, nb, taps_stride, radius, htaps_stride, hradius)) return rc;
    if ((const void*)back == score_prev || (const void*)back == prev_stats || back == cell || back == bin)
        return ccvpe_fail(CCVPE_EINVAL, "back must not alias score_prev, prev_stats, cell or bin");
    if ((uintptr_t)score_prev & 15) return ccvpe_fail(CCVPE_EINVAL, "score_prev must be 16-byte aligned");
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    TrackJointViterbiBackParams p{};
    p.score_prev = score_prev; p.prev_stats = prev_stats; p.cell = cell; p.bin = bin; p.shift = shift; p.taps = taps; p.taps_stride = taps_stride;
    p.radius = radius; p.turn_deg = turn_deg; p.htaps = htaps; p.htaps_stride = htaps_stride; p.hradius = hradius; p.floor = floor;
    p.back = back; p.B = batch; p.nb = nb;
    launch_track_joint_viterbi_back(p, (hipStream_t)stream);
    return launch_status("track_joint_viterbi_back launch");
}

// ------------------------------------------------------------------------------------------------
// Credible regions: the radix select of kernels_credible.hip over a stored map (ccvpe_belief_credible, on the prior
// scratch), behind the logits tail on the prior scratch (ccvpe_postprocess_credible), or as pose.credible behind pose.argmax in
// plans of their own (PlanKey::credible; every other launch keeps the name and tuning entry of the argmax pose plan).
// ------------------------------------------------------------------------------------------------
// the levels: host memory, read here and carried by value from here on
static int check_credible_levels(const float* levels, int32_t n_levels) {
    if (n_levels < 1 || n_levels > CRED_MAX_LEVELS) return ccvpe_fail(CCVPE_EINVAL, "n_levels must be in 1 .. %d, got %d", CRED_MAX_LEVELS, n_levels);
    for (int32_t j = 0; j < n_levels; ++j)
        if (!(std::isfinite(levels[j]) && levels[j] > 0.f && levels[j] <= 1.f))
            return ccvpe_fail(CCVPE_EINVAL, "levels[%d] = %g is not a finite level in (0, 1]", j, (double)levels[j]);
    return 0;
}
// cred and level_map against each other and against every other buffer of the call (null entries: absent)
struct CredOther { const char* name; const void* ptr; };
static int check_credible_alias(const void* cred, const void* level_map, std::initializer_list<CredOther> others) {
    if (level_map && level_map == cred) return ccvpe_fail(CCVPE_EINVAL, "level_map must not alias cred");
    for (const CredOther& o : others) {
        if (o.ptr && o.ptr == cred) return ccvpe_fail(CCVPE_EINVAL, "cred must not alias %s", o.name);
        if (o.ptr && level_map && o.ptr == level_map) return ccvpe_fail(CCVPE_EINVAL, "level_map must not alias %s", o.name);
    }
    return 0;
}
static void credible_call(TailCall& t, const float* levels, int32_t n_levels, const int32_t* probe, float* cred, uint8_t* level_map) {
    t.cred = cred; t.cred_levels = n_levels; t.cred_probe = probe; t.cred_map = level_map;
    for (int32_t j = 0; j < n_levels; ++j) t.cred_level[j] = levels[j];
}
// what the forms with rows share behind their own pointers: the levels, the prior's stride, the optional posterior's aliasing
static int check_credible_tail(const float* levels, int32_t n_levels, const float* log_prior, int64_t prior_stride) {
    if (int rc = check_credible_levels(levels, n_levels)) return rc;
    if (log_prior) if (int rc = check_prior_stride(prior_stride)) return rc;
    return 0;
}

int ccvpe_belief_credible(ccvpe_handle h, const float* belief, int32_t batch, const float* levels, int32_t n_levels, const int32_t* probe,
                          float* cred, uint8_t* level_map, void* stream) {
    if (!belief) return ccvpe_fail(CCVPE_EINVAL, "null belief");
    if (!levels) return ccvpe_fail(CCVPE_EINVAL, "null levels");
    if (!cred) return ccvpe_fail(CCVPE_EINVAL, "null cred");
    if (int rc = check_credible_levels(levels, n_levels)) return rc;
    if (batch <= 0 || batch > PP_MAX_BATCH) return ccvpe_fail(CCVPE_EINVAL, "batch must be in 1 .. %d, got %d", PP_MAX_BATCH, batch);
    if (((uintptr_t)belief & 3) != 0) return ccvpe_fail(CCVPE_EINVAL, "belief must be 4-byte aligned");
    if (int rc = check_credible_alias(cred, level_map, {{"belief", belief}, {"probe", probe}})) return rc;
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    if (int rc = ensure_scratch(h->prior_scratch, batch, prior_scratch_bytes, "prior post-processing scratch")) return rc;
    const TailBuffers w = scratch_buffers(h->prior_scratch, nullptr, nullptr);
    TailCall t;
    credible_call(t, levels, n_levels, probe, cred, level_map);
    issue_pose_credible(w, t, belief, batch, (hipStream_t)stream);
    return launch_status("belief_credible launch");
}

int ccvpe_postprocess_credible(ccvpe_handle h, const float* logits, const float* ori, int32_t batch, const float* log_prior,
                               int64_t prior_stride, const float* levels, int32_t n_levels, const int32_t* probe, float* rows, float* cred,
                               uint8_t* level_map, float* posterior, void* stream) {
    if (!logits) return ccvpe_fail(CCVPE_EINVAL, "null logits");
    if (!ori) return ccvpe_fail(CCVPE_EINVAL, "null ori");
    if (!levels) return ccvpe_fail(CCVPE_EINVAL, "null levels");
    if (!rows) return ccvpe_fail(CCVPE_EINVAL, "null rows");
    if (!cred) return ccvpe_fail(CCVPE_EINVAL, "null cred");
    if (int rc = check_credible_tail(levels, n_levels, log_prior, prior_stride)) return rc;
    if (batch <= 0 || batch > PP_MAX_BATCH) return ccvpe_fail(CCVPE_EINVAL, "batch must be in 1 .. %d, got %d", PP_MAX_BATCH, batch);
    if (int rc = check_credible_alias(cred, level_map, {{"logits", logits}, {"ori", ori}, {"log_prior", log_prior}, {"probe", probe}, {"rows", rows},
                                                        {"posterior", posterior}})) return rc;
    if (posterior && log_prior && (const float*)log_prior == posterior) return ccvpe_fail(CCVPE_EINVAL, "posterior must not alias log_prior");
    if (posterior && posterior == rows) return ccvpe_fail(CCVPE_EINVAL, "posterior must not alias rows");
    if (posterior && posterior == logits) return ccvpe_fail(CCVPE_EINVAL, "posterior must not alias logits");
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    TailCall t;
    t.rows = rows; t.log_prior = log_prior; t.prior_stride = log_prior ? prior_stride : 0; t.posterior = posterior;
    credible_call(t, levels, n_levels, probe, cred, level_map);
    if (int rc = run_logits_tail(h, logits, ori, batch, t, (hipStream_t)stream)) return rc;
    return launch_status("postprocess_credible launch");
}

int ccvpe_localize_credible(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const float* sat, int32_t batch,
                            const float* log_prior, int64_t prior_stride, const float* levels, int32_t n_levels, const int32_t* probe,
                            float* rows, float* cred, uint8_t* level_map, float* posterior, void* stream) {
    if (!grd) return ccvpe_fail(CCVPE_EINVAL, "null grd");
    if (!sat) return ccvpe_fail(CCVPE_EINVAL, "null sat");
    if (!levels) return ccvpe_fail(CCVPE_EINVAL, "null levels");
    if (!rows) return ccvpe_fail(CCVPE_EINVAL, "null rows");
    if (!cred) return ccvpe_fail(CCVPE_EINVAL, "null cred");
    if (int rc = check_credible_tail(levels, n_levels, log_prior, prior_stride)) return rc;
    if (int rc = check_credible_alias(cred, level_map, {{"grd", grd}, {"sat", sat}, {"log_prior", log_prior}, {"probe", probe}, {"rows", rows},
                                                        {"posterior", posterior}})) return rc;
    if (posterior && log_prior && (const float*)log_prior == posterior) return ccvpe_fail(CCVPE_EINVAL, "posterior must not alias log_prior");
    if (posterior && posterior == rows) return ccvpe_fail(CCVPE_EINVAL, "posterior must not alias rows");
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.sat = sat; fc.tail.rows = rows; fc.tail.log_prior = log_prior; fc.tail.prior_stride = log_prior ? prior_stride : 0; fc.tail.posterior = posterior;
    credible_call(fc.tail, levels, n_levels, probe, cred, level_map);
    return run_forward(h, fc);
}

int ccvpe_localize_credible_cached_indexed(ccvpe_handle h, const float* grd, int32_t grd_h, int32_t grd_w, const void* cache, int32_t n_tiles,
                                           const int32_t* tile_index, int32_t batch, const float* log_prior, int64_t prior_stride,
                                           const float* levels, int32_t n_levels, const int32_t* probe, float* rows, float* cred,
                                           uint8_t* level_map, float* posterior, void* stream) {
    if (!grd) return ccvpe_fail(CCVPE_EINVAL, "null grd");
    if (!cache) return ccvpe_fail(CCVPE_EINVAL, "null cache");
    if (!levels) return ccvpe_fail(CCVPE_EINVAL, "null levels");
    if (!rows) return ccvpe_fail(CCVPE_EINVAL, "null rows");
    if (!cred) return ccvpe_fail(CCVPE_EINVAL, "null cred");
    if (int rc = check_credible_tail(levels, n_levels, log_prior, prior_stride)) return rc;
    if (int rc = check_credible_alias(cred, level_map, {{"grd", grd}, {"cache", cache}, {"log_prior", log_prior}, {"probe", probe}, {"rows", rows},
                                                        {"posterior", posterior}})) return rc;
    if (int rc = check_cached_args(grd, cache, n_tiles, tile_index, batch, rows)) return rc;
    if (posterior && log_prior && (const float*)log_prior == posterior) return ccvpe_fail(CCVPE_EINVAL, "posterior must not alias log_prior");
    if (posterior && posterior == rows) return ccvpe_fail(CCVPE_EINVAL, "posterior must not alias rows");
    if (!h) return ccvpe_fail(CCVPE_EINVAL, "null handle");
    ForwardCall fc = forward_call(grd, grd_h, grd_w, batch, stream);
    fc.cache = (const float*)cache; fc.tile_index = tile_index; fc.n_tiles = n_tiles;
    fc.tail.rows = rows; fc.tail.log_prior = log_prior; fc.tail.prior_stride = log_prior ? prior_stride : 0; fc.tail.posterior = posterior;
    credible_call(fc.tail, levels, n_levels, probe, cred, level_map);
    return run_forward(h, fc);
}

int ccvpe_preprocess(const uint8_t* hwc, int32_t batch, int32_t H, int32_t W, const int32_t* shift, int32_t crop_w,
                     const float mean[3], const float stdv[3], float* out_nchw, void* stream) {
    if (!hwc || !out_nchw || !mean || !stdv) return ccvpe_fail(CCVPE_EINVAL, "null argument");
    if (batch <= 0 || H <= 0 || W <= 0 || crop_w <= 0 || crop_w > W) return ccvpe_fail(CCVPE_EINVAL, "bad geometry");
    PreprocParams p{};
    p.in = hwc; p.B = batch; p.H = H; p.W = W; p.crop_w = crop_w; p.shift = shift; p.out = out_nchw;
    for (int c = 0; c < 3; ++c) { p.mean[c] = mean[c]; p.stdv[c] = stdv[c]; }
    launch_preprocess(p, (hipStream_t)stream);
    return launch_status("preprocess launch");
}


int ccvpe_preprocess_resize(const uint8_t* hwc, int32_t batch, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w,
                            const int32_t* shift, int32_t crop_w, const float mean[3], const float stdv[3], uint8_t* scratch,
                            float* out_nchw, void* stream) {
    if (!hwc || !out_nchw || !mean || !stdv) return ccvpe_fail(CCVPE_EINVAL, "null argument");
    if (batch <= 0 || in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0 || crop_w <= 0 || crop_w > out_w) return ccvpe_fail(CCVPE_EINVAL, "bad geometry");
    if (in_w != out_w && !scratch) return ccvpe_fail(CCVPE_EINVAL, "scratch of batch*in_h*out_w*3 bytes is required when the width changes");
    if ((double)batch * in_h * std::max(in_w, out_w) * 3 >= 2147483647.0 * 2) return ccvpe_fail(CCVPE_EINVAL, "image batch too large");
    ResizeParams p{};
    p.in = hwc; p.B = batch; p.IH = in_h; p.IW = in_w; p.OH = out_h; p.OW = out_w; p.crop_w = crop_w; p.tmp = scratch; p.shift = shift; p.out = out_nchw;
    for (int c = 0; c < 3; ++c) { p.mean[c] = mean[c]; p.stdv[c] = stdv[c]; }
    if (launch_resize(p, (hipStream_t)stream) != 0) return ccvpe_fail(CCVPE_EINVAL, "down-scaling factors above 8 are not supported (%dx%d -> %dx%d)", in_h, in_w, out_h, out_w);
    return launch_status("resize launch");
}

int ccvpe_preprocess_affine(const uint8_t* hwc, int32_t batch, int32_t H, int32_t W, const double* matrices, const int32_t* filters,
                            int32_t n_stages, int32_t top, int32_t left, int32_t out_h, int32_t out_w, const float mean[3],
                            const float stdv[3], float* out_nchw, void* stream) {
    if (!hwc || !matrices || !filters || !mean || !stdv || !out_nchw) return ccvpe_fail(CCVPE_EINVAL, "null argument");
    if (n_stages < 1 || n_stages > WARP_MAX_STAGES) return ccvpe_fail(CCVPE_EINVAL, "%d stages (1..%d are supported)", n_stages, WARP_MAX_STAGES);
    unsigned bil = 0;
    int n_bil = 0;
    for (int s = 0; s < n_stages; ++s) {
        if (filters[s] == CCVPE_RESAMPLE_BILINEAR) { bil |= 1u << s; ++n_bil; }
        else if (filters[s] != CCVPE_RESAMPLE_NEAREST) return ccvpe_fail(CCVPE_EINVAL, "stage %d: unknown filter %d (NEAREST 0 or BILINEAR 2)", s, filters[s]);
    }
    if (n_bil > WARP_MAX_BILINEAR) return ccvpe_fail(CCVPE_EINVAL, "%d BILINEAR stages (at most %d)", n_bil, WARP_MAX_BILINEAR);
    if (batch <= 0 || batch > 65535) return ccvpe_fail(CCVPE_EINVAL, "batch %d out of range (1..65535)", batch);
    if (H <= 0 || W <= 0 || H > 16384 || W > 16384) return ccvpe_fail(CCVPE_EINVAL, "canvas %d x %d out of range (1..16384 per side)", H, W);
    if (out_h <= 0 || out_w <= 0 || top < 0 || left < 0 || top > H - out_h || left > W - out_w)
        return ccvpe_fail(CCVPE_EINVAL, "crop (top %d, left %d, %d x %d) outside the %d x %d canvas", top, left, out_h, out_w, H, W);
    WarpParams p{};
    p.in = hwc; p.mat = matrices; p.B = batch; p.H = H; p.W = W; p.n = n_stages; p.bilinear = bil;
    p.top = top; p.left = left; p.out_h = out_h; p.out_w = out_w; p.out = out_nchw;
    for (int c = 0; c < 3; ++c) { p.mean[c] = mean[c]; p.stdv[c] = stdv[c]; }
    if (launch_warp(p, (hipStream_t)stream) != 0) return ccvpe_fail(CCVPE_EINVAL, "no kernel for this stage pattern");
    return launch_status("affine launch");
}

int ccvpe_preprocess_window_resize(const uint8_t* map_hwc, int32_t map_h, int32_t map_w, const int32_t* origins, int32_t batch,
                                   int32_t win_h, int32_t win_w, int32_t out_h, int32_t out_w, const float mean[3], const float stdv[3],
                                   uint8_t* scratch, float* out_nchw, void* stream) {
    if (!map_hwc || !origins || !mean || !stdv || !scratch || !out_nchw) return ccvpe_fail(CCVPE_EINVAL, "null argument");
    if (map_h <= 0 || map_w <= 0 || batch <= 0 || win_h <= 0 || win_w <= 0 || out_h <= 0 || out_w <= 0) return ccvpe_fail(CCVPE_EINVAL, "bad geometry");
    if (win_w > 8 * out_w || win_h > 8 * out_h)
        return ccvpe_fail(CCVPE_EINVAL, "down-scaling factors above 8 are not supported (%dx%d -> %dx%d)", win_h, win_w, out_h, out_w);
    if ((double)batch * win_h * out_w * 3 >= 2147483647.0 * 2 || (double)batch * 3 * out_h * out_w >= 2147483647.0 * 2)
        return ccvpe_fail(CCVPE_EINVAL, "window batch too large");
    ResizeParams p{};
    p.in = map_hwc; p.B = batch; p.IH = win_h; p.IW = win_w; p.OH = out_h; p.OW = out_w; p.crop_w = out_w; p.tmp = scratch; p.out = out_nchw;
    p.origin = origins; p.map_h = map_h; p.map_w = map_w;
    for (int c = 0; c < 3; ++c) { p.mean[c] = mean[c]; p.stdv[c] = stdv[c]; }
    if (launch_resize(p, (hipStream_t)stream) != 0) return ccvpe_fail(CCVPE_EINVAL, "down-scaling factors above 8 are not supported");
    return launch_status("window resize launch");
}

int ccvpe_debug_dump_plan(ccvpe_handle h, const char* path) {
    if (!h || !path) return ccvpe_fail(CCVPE_EINVAL, "null argument");
    Plan* pl = h->last_plan;
    if (!pl) return ccvpe_fail(CCVPE_ESTATE, "no forward has run on this handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipDeviceSynchronize());
    const size_t n = pl->size.size();
    unsigned long long* d = nullptr;
    HIPCHK(hipMalloc((void**)&d, n * sizeof(unsigned long long)));
    HIPCHK(hipMemset(d, 0, n * sizeof(unsigned long long)));
    for (size_t id = 0; id < n; ++id) {
        if (pl->size[id] == 0) continue;
        const int blocks = (int)std::min<size_t>((pl->size[id] + 255) / 256, 2048);
        CCVPE_LAUNCH(checksum_kernel, dim3(blocks), dim3(256), 0, nullptr, reinterpret_cast<const uint32_t*>(h->arena + pl->off[id]), pl->size[id], d + id);
    }
    std::vector<unsigned long long> sums(n);
    hipError_t e = hipMemcpy(sums.data(), d, n * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return ccvpe_fail(CCVPE_EHIP, "checksum copy failed: %s", hipGetErrorString(e));
    FILE* f = std::fopen(path, "w");
    if (!f) return ccvpe_fail(CCVPE_EINVAL, "cannot open %s", path);
    std::fprintf(f, "# plan B=%d grd=%dx%d mode=%d two_streams=%d tensors=%zu arena_floats=%zu\n", pl->key.B, pl->key.gh, pl->key.gw, pl->key.mode, (int)pl->two_streams, n, pl->total);
    for (size_t i = 0; i < pl->ops.size(); ++i) {
        const Op& op = pl->ops[i];
        std::fprintf(f, "op %zu %s stream=%d wait=%d signal=%d tile=%s", i, op.name.c_str(), op.stream, op.wait_on.empty() ? -1 : op.wait_on[0], (int)op.signal,
                     op.tile ? conv_tile_name(*op.tile) : "-");
        if (op.tile && (*op.tile >> 8) == 255) std::fprintf(f, "_tailsplit");
        else if (op.tile && (*op.tile >> 8) > SPLIT_FUSED) std::fprintf(f, "_splitk%dr", (*op.tile >> 8) - SPLIT_FUSED);
        else if (op.tile && (*op.tile >> 8) > 1) std::fprintf(f, "_splitk%d", *op.tile >> 8);
        for (int id : op.uses) std::fprintf(f, " t%d[off=%zu,n=%zu]=%016llx", id, pl->off[id], pl->size[id], sums[id]);
        std::fprintf(f, "\n");
    }
    if (h->snap[0]) {   // CCVPE_DIAG_SNAP: what the named launch's tensors held right before / right after it, in stream order
        for (int which = 0; which < 2; ++which) {
            std::fprintf(f, "snap_%s %s", which ? "after" : "before", h->sw.diag_snap.c_str());
            for (auto& e : h->snap_layout) {
                unsigned long long* dd = nullptr;
                unsigned long long v = 0;
                if (hipMalloc((void**)&dd, sizeof(v)) == hipSuccess) {
                    (void)hipMemset(dd, 0, sizeof(v));
                    const int blocks = (int)std::min<size_t>((pl->size[e.first] + 255) / 256, 2048);
                    CCVPE_LAUNCH(checksum_kernel, dim3(blocks), dim3(256), 0, nullptr, reinterpret_cast<const uint32_t*>(h->snap[which] + e.second), pl->size[e.first], dd);
                    (void)hipMemcpy(&v, dd, sizeof(v), hipMemcpyDeviceToHost);
                    (void)hipFree(dd);
                }
                std::fprintf(f, " t%d=%016llx", e.first, v);
            }
            std::fprintf(f, "\n");
        }
    }
    std::fclose(f);
    return 0;
}

int ccvpe_op_num_tiles(void) { return conv_num_tiles(); }
const char* ccvpe_op_tile_name(int32_t tile) { return conv_tile_name(tile); }

// The body of both convolution hooks: argument checks (all before the first launch), the packer that serves ccvpe_create, the launch
// parameters a plan would build for this form, one launch (plus `iters` timed ones).  wino_strict: the old hook's contract - a Winograd
// id on a layer the tile does not take is an error; ccvpe_op_conv2d_ex reports the fallback instead.
static int op_conv_run(const ccvpe_op_conv_desc& d, bool wino_strict, hipStream_t st) {
    const int B = d.B, H = d.H, W = d.W, Cin = d.Cin, Cout = d.Cout, KH = d.KH, KW = d.KW, stride = d.stride, pad = d.pad;
    if (!d.in || !d.w) return ccvpe_fail(CCVPE_EINVAL, "null argument");
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cin % 8 || Cout <= 0 || KH <= 0 || KW <= 0 || stride <= 0 || pad < 0)
        return ccvpe_fail(CCVPE_EINVAL, "bad conv geometry (Cin must be a multiple of 8)");
    const bool deconv = d.mode == CCVPE_OP_DECONV;
    if (d.mode != CCVPE_OP_CONV && !deconv) return ccvpe_fail(CCVPE_EINVAL, "unknown mode %d", d.mode);
    if (deconv && (KH != 2 || KW != 2 || stride != 2 || pad != 0)) return ccvpe_fail(CCVPE_EINVAL, "the transposed conv is 2x2, stride 2, pad 0");
    const int in_ld = d.in_ld ? d.in_ld : Cin;
    if (in_ld < Cin || in_ld % 4) return ccvpe_fail(CCVPE_EINVAL, "in_ld must be >= Cin and a multiple of 4");
    // GEMM rows: output pixels of a conv, input pixels of a transposed conv (whose four (dy, dx) column groups are shuffled on store)
    const int OH = deconv ? H : (H + 2 * pad - KH) / stride + 1, OW = deconv ? W : (W + 2 * pad - KW) / stride + 1;
    if (OH <= 0 || OW <= 0) return ccvpe_fail(CCVPE_EINVAL, "empty output");
    const int N = deconv ? 4 * Cout : Cout;
    const double opix = (double)B * OH * OW * (deconv ? 4 : 1);
    if ((double)B * H * W * in_ld >= 2147483647.0 || opix * Cout >= 2147483647.0) return ccvpe_fail(CCVPE_EINVAL, "tensor exceeds 2^31 elements");
    if (d.gate && (KH != 1 || KW != 1 || stride != 1 || pad != 0 || deconv)) return ccvpe_fail(CCVPE_EINVAL, "a gate goes with a 1x1 / stride 1 / pad 0 conv only");
    if (d.resid) {
        if (deconv) return ccvpe_fail(CCVPE_EINVAL, "no residual on a transposed conv");
        if (d.act != 0) return ccvpe_fail(CCVPE_EINVAL, "a residual goes with act 0 only (no plan adds one behind an activation)");
        if (d.resid_ld < N) return ccvpe_fail(CCVPE_EINVAL, "resid_ld must be >= Cout");
        if ((double)B * OH * OW * d.resid_ld >= 2147483647.0) return ccvpe_fail(CCVPE_EINVAL, "tensor exceeds 2^31 elements");
    }
    if (d.ndst < 1 || d.ndst > 3) return ccvpe_fail(CCVPE_EINVAL, "ndst must be 1 .. 3");
    for (int i = 0; i < d.ndst; ++i) {
        if (!d.dst[i].ptr) return ccvpe_fail(CCVPE_EINVAL, "null destination %d", i);
        if (d.dst[i].coff < 0 || d.dst[i].ld <= 0 || (long long)d.dst[i].coff + Cout > d.dst[i].ld) return ccvpe_fail(CCVPE_EINVAL, "destination %d: coff + Cout must be <= ld", i);
        if (opix * d.dst[i].ld >= 2147483647.0) return ccvpe_fail(CCVPE_EINVAL, "tensor exceeds 2^31 elements");
    }
    const int tile = d.tile;
    const int taps = deconv ? 1 : KH * KW;
    const size_t nw = (size_t)Cout * Cin * KH * KW;
    std::vector<float> hw(nw), hb(N, 0.f);
    HIPCHK(hipMemcpy(hw.data(), d.w, nw * sizeof(float), hipMemcpyDefault));
    if (d.bias) {
        HIPCHK(hipMemcpy(hb.data(), d.bias, Cout * sizeof(float), hipMemcpyDefault));
        if (deconv) for (int q = 1; q < 4; ++q) std::copy(hb.begin(), hb.begin() + Cout, hb.begin() + (size_t)q * Cout);
    }
    ccvpe_handle_s tmp;   // only its dev_allocs list, precision flag and packer switches are used by the packer
    tmp.sw = read_switches();
    tmp.cfg.reserved[0] = 1;   // also pack the bf16x3 planes so every tile id can be exercised
    PackedConv pc;
    int rc;
    if (deconv)   // ConvTranspose2d weight [Cin][Cout][2][2] -> rows n = (dy*2+dx)*Cout + o of a 1x1 GEMM, as build_decoder packs a level
        rc = pack_conv(&tmp, pc, N, 1, Cin, Cin, identity_map(Cin),
                       [&](int n, int, int c) { const int q = n / Cout, o = n % Cout; return hw[((size_t)c * Cout + o) * 4 + q]; }, hb, 1, 1);
    else
        rc = pack_conv(&tmp, pc, Cout, taps, Cin, Cin, identity_map(Cin),
                       [&](int n, int t, int c) { return hw[((size_t)n * Cin + c) * taps + t]; }, hb, KH, KW);
    auto cleanup = [&]() { for (void* p : tmp.dev_allocs) (void)hipFree(p); };
    if (rc) { cleanup(); return rc; }
    ConvParams p = deconv ? conv_params(pc, d.in, in_ld, B, H, W, H, W, 1, 0, 0, d.act) : conv_params(pc, d.in, in_ld, B, H, W, OH, OW, stride, pad, pad, d.act);
    if (deconv) { p.mode = MODE_DECONV; p.deconv_cout = Cout; }
    p.gate = d.gate;
    if (d.resid) { p.resid = d.resid; p.resid_ld = d.resid_ld; }
    p.ndst = d.ndst;
    for (int i = 0; i < d.ndst; ++i) p.dst[i] = {d.dst[i].ptr, d.dst[i].ld, d.dst[i].coff};
    if (((tile >> 8) & 0xff) > 1) {   // tile word = id | (split-K << 8): give the launch a slab (and ticket counters: 255 and the codes above SPLIT_FUSED reduce themselves)
        int sk = (tile >> 8) & 0xff;
        if (sk > SPLIT_FUSED && sk != 255) sk -= SPLIT_FUSED;
        {
            void* dd = nullptr;
            if (hipMalloc(&dd, CONV_TICKETS * sizeof(unsigned)) != hipSuccess || hipMemset(dd, 0, CONV_TICKETS * sizeof(unsigned)) != hipSuccess) { cleanup(); return ccvpe_fail(CCVPE_ENOMEM, "ticket counters"); }
            tmp.dev_allocs.push_back(dd);
            tmp.dev_alloc_bytes.push_back(CONV_TICKETS * sizeof(unsigned));
            p.tickets = (unsigned*)dd;
        }
        const size_t fl = (size_t)(sk == 255 ? 8 : sk) * p.M * p.N;   // 255 = F(4x4) tail split: its slab is a fraction of 8 full ones
        void* dd = nullptr;
        if (hipMalloc(&dd, fl * sizeof(float)) != hipSuccess) { cleanup(); return ccvpe_fail(CCVPE_ENOMEM, "split-K slab"); }
        tmp.dev_allocs.push_back(dd);
        tmp.dev_alloc_bytes.push_back(fl * sizeof(float));
        p.partial = (float*)dd; p.partial_floats = fl;
    }
    const ConvTile* t = conv_tile(tile);
    const int runs = t ? (conv_tile_runs(*t, p) ? 1 : 0) : -1;
    if (d.requested_runs) *d.requested_runs = runs;
    if (wino_strict && t && t->family == TILE_WINO && !runs) { cleanup(); return ccvpe_fail(CCVPE_EINVAL, "layer is not Winograd-shaped (3x3, stride 1, pad 1, W %% 16 == 0, H %% 16 == 0, output channels a multiple of 4; F(4x4): >= 40 of them)"); }
    (void)conv_tile_last();
    if (launch_conv_igemm(p, tile, st) != 0) { cleanup(); return ccvpe_fail(CCVPE_EINVAL, "unsupported conv geometry (KH*KW <= 16, Cin %% 8 == 0)"); }
    const int last = conv_tile_last();   // (reading it clears it: the timed launches below leave nothing behind)
    if (d.ran_tile) *d.ran_tile = last & 0xff;
    if (d.ran_split) *d.ran_split = (last >> 8) & 0xff;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && d.iters > 0 && d.ms) {
        hipEvent_t e0, e1;
        (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
        (void)hipEventRecord(e0, st);
        for (int i = 0; i < d.iters; ++i) launch_conv_igemm(p, tile, st);
        (void)hipEventRecord(e1, st);
        (void)hipEventSynchronize(e1);
        float tm = 0.f;
        (void)hipEventElapsedTime(&tm, e0, e1);
        *d.ms = tm / d.iters;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        (void)conv_tile_last();
    }
    hipError_t e2 = hipStreamSynchronize(st);
    cleanup();
    if (e != hipSuccess) return ccvpe_fail(CCVPE_EHIP, "conv launch failed: %s", hipGetErrorString(e));
    if (e2 != hipSuccess) return ccvpe_fail(CCVPE_EHIP, "conv execution failed: %s", hipGetErrorString(e2));
    return 0;
}

int ccvpe_op_conv2d_ex(const ccvpe_op_conv_desc* d, void* stream) {
    if (!d) return ccvpe_fail(CCVPE_EINVAL, "null argument");
    return op_conv_run(*d, false, (hipStream_t)stream);
}

int ccvpe_op_conv2d(const float* in, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w, const float* bias,
                    int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t act, int32_t tile,
                    float* out, int32_t iters, float* ms, void* stream) {
    if (!in || !w || !out) return ccvpe_fail(CCVPE_EINVAL, "null argument");
    ccvpe_op_conv_desc d{};
    d.in = in; d.B = B; d.H = H; d.W = W; d.Cin = Cin; d.in_ld = Cin; d.w = w; d.bias = bias;
    d.Cout = Cout; d.KH = KH; d.KW = KW; d.stride = stride; d.pad = pad; d.act = act; d.tile = tile; d.mode = CCVPE_OP_CONV;
    d.ndst = 1; d.dst[0].ptr = out; d.dst[0].ld = Cout; d.dst[0].coff = 0;
    d.iters = iters; d.ms = ms;
    return op_conv_run(d, true, (hipStream_t)stream);
}

int ccvpe_op_level1(const float* in, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t score, const float* wd, const float* bd,
                    const float* wa, const float* ba, const float* wt, const float* bt, int32_t Cout, int32_t tile, float* out, void* stream) {
    if (!in || !wd || !bd || !wa || !ba || !wt || !bt || !out) return ccvpe_fail(CCVPE_EINVAL, "null argument");
    const int cd = Cin - (score ? 1 : 0);
    if (B <= 0 || H <= 0 || W <= 0 || H % 16 || W % 16 || (Cout != 1 && Cout != 2) || cd <= 0 || cd % 4 || tile < 0 || (tile & 0xff) > 1 || ((tile >> 8) != 0 && (tile >> 8) < 8))
        return ccvpe_fail(CCVPE_EINVAL, "bad level-1 geometry (H, W multiples of 16, Cout 1 or 2, descriptor channels a multiple of 4, tile 0 or 1, workgroup cap 0 or >= 8)");
    if ((double)B * H * W * 16 >= 2147483647.0) return ccvpe_fail(CCVPE_EINVAL, "tensor exceeds 2^31 elements");
    std::vector<float> hwd((size_t)Cin * 64), hbd(16), hwa(16 * 16 * 9), hba(16), hwt((size_t)Cout * 16 * 9), hbt(Cout);
    HIPCHK(hipMemcpy(hwd.data(), wd, hwd.size() * sizeof(float), hipMemcpyDefault));
    HIPCHK(hipMemcpy(hbd.data(), bd, hbd.size() * sizeof(float), hipMemcpyDefault));
    HIPCHK(hipMemcpy(hwa.data(), wa, hwa.size() * sizeof(float), hipMemcpyDefault));
    HIPCHK(hipMemcpy(hba.data(), ba, hba.size() * sizeof(float), hipMemcpyDefault));
    HIPCHK(hipMemcpy(hwt.data(), wt, hwt.size() * sizeof(float), hipMemcpyDefault));
    HIPCHK(hipMemcpy(hbt.data(), bt, hbt.size() * sizeof(float), hipMemcpyDefault));
    ccvpe_handle_s tmp;   // only its dev_allocs list is used
    DecoderW d;
    auto cleanup = [&]() { for (void* p : tmp.dev_allocs) (void)hipFree(p); };
    int rc = compose_level1(&tmp, d, hwd, hbd, hwa, hba, Cin, score ? 1 : 0);
    if (!rc) rc = pack_level1_tail(&tmp, d, hwt, hbt, Cout);
    if (rc) { cleanup(); return rc; }
    if (!level1_supported(d.l1_cxp)) { cleanup(); return ccvpe_fail(CCVPE_EINVAL, "the fused level takes up to 64 input channels"); }
    Level1Params lp = level1_params(d, d.l1_cx, B, Cout, Cout == 2);
    lp.x = in; lp.H = H; lp.W = W; lp.out = out; lp.raw = nullptr; lp.tile = tile & 0xff; lp.max_wg = tile >> 8;
    hipStream_t st = (hipStream_t)stream;
    launch_level1(lp, st);
    hipError_t e = hipGetLastError();
    hipError_t e2 = hipStreamSynchronize(st);
    cleanup();
    if (e != hipSuccess) return ccvpe_fail(CCVPE_EHIP, "level-1 launch failed: %s", hipGetErrorString(e));
    if (e2 != hipSuccess) return ccvpe_fail(CCVPE_EHIP, "level-1 execution failed: %s", hipGetErrorString(e2));
    return level1_tile(lp);
}

int ccvpe_op_deconv_k2s2(const float* in, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t in_ld, const float* w, const float* bias, int32_t Cout,
                         float* out, int32_t ld, int32_t coff, int32_t cw, void* stream) {
    if (!in || !w || !out) return ccvpe_fail(CCVPE_EINVAL, "null argument");
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cin % 8 || Cout <= 0 || cw < Cout || in_ld < Cin)
        return ccvpe_fail(CCVPE_EINVAL, "bad transposed-conv geometry (Cin a multiple of 8, in_ld >= Cin, cw >= Cout)");
    std::vector<float> hw((size_t)Cin * Cout * 4), b1(Cout, 0.f), hb(4 * (size_t)cw, 0.f);
    HIPCHK(hipMemcpy(hw.data(), w, hw.size() * sizeof(float), hipMemcpyDefault));
    if (bias) HIPCHK(hipMemcpy(b1.data(), bias, Cout * sizeof(float), hipMemcpyDefault));
    for (int q = 0; q < 4; ++q) std::copy(b1.begin(), b1.end(), hb.begin() + (size_t)q * cw);   // (columns past Cout: zero)
    // the kernel's form is chosen from the sizes and from which input channels have a weight that is not zero
    std::vector<unsigned char> live(Cin, 0);
    for (int c = 0; c < Cin; ++c)
        for (int i = 0; i < Cout * 4 && !live[c]; ++i) live[c] = hw[(size_t)c * Cout * 4 + i] != 0.f;
    DeconvK2S2Params kp{};
    kp.B = B; kp.H = H; kp.W = W; kp.Cin = Cin; kp.in_ld = in_ld; kp.Kpad = round_up(Cin, 32);
    kp.ld = ld; kp.coff = coff; kp.cw = cw;
    if (!deconv_k2s2_prepare(kp, live.data()))
        return ccvpe_fail(CCVPE_EINVAL, "deconv_k2s2_kernel does not take these sizes (cw a multiple of 16 up to 80, in_ld, ld and coff multiples of 4, coff + cw <= ld, "
                                        "at most 192 live input channels, weights of two taps within the LDS)");
    ccvpe_handle_s tmp;   // only its dev_allocs list and packer switches are used by the packer
    tmp.sw = read_switches();
    PackedConv pc;
    // ConvTranspose2d weight [Cin][Cout][2][2] -> rows n = (dy*2+dx)*cw + o of a 1x1 GEMM, zero rows past Cout: as build_decoder packs a level
    int rc = pack_conv(&tmp, pc, 4 * cw, 1, Cin, Cin, identity_map(Cin),
                       [&](int n, int, int c) { const int q = n / cw, o = n % cw; return o < Cout ? hw[((size_t)c * Cout + o) * 4 + q] : 0.f; }, hb, 1, 1);
    auto cleanup = [&]() { for (void* p : tmp.dev_allocs) (void)hipFree(p); };
    if (rc) { cleanup(); return rc; }
    if (pc.Kpad < Cin || pc.N != 4 * cw) { cleanup(); return ccvpe_fail(CCVPE_ESTATE, "unexpected packed form"); }
    kp.Kpad = pc.Kpad;
    kp.x = in; kp.wpk = pc.w; kp.bias = pc.bias; kp.out = out;
    hipStream_t st = (hipStream_t)stream;
    launch_deconv_k2s2(kp, st);
    hipError_t e = hipGetLastError();
    hipError_t e2 = hipStreamSynchronize(st);
    cleanup();
    if (e != hipSuccess) return ccvpe_fail(CCVPE_EHIP, "transposed-conv launch failed: %s", hipGetErrorString(e));
    if (e2 != hipSuccess) return ccvpe_fail(CCVPE_EHIP, "transposed-conv execution failed: %s", hipGetErrorString(e2));
    return kp.taps;
}

}  // extern "C"

