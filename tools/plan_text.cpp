// The launch list of every plan form as text, without a device (tests/test_plan_text_cpu.py).
//
//   hipcc -std=c++17 tools/plan_text.cpp -Iccvpe_amd/csrc -Lccvpe_amd/csrc -lccvpe_hip -Wl,-rpath,$PWD/ccvpe_amd/csrc -o plan_text
//   plan_text                 one line per plan: label, return code, ops, tensors, total, ticket words, FNV-1a hash of its full text
//   plan_text --compact       one line per (variant, streams, fusion, flavour, batch): the low 32 bits of its 40 plans' hashes, in
//                             the order modes 0-4 x forms - the form tests/plan_text_parent.txt is recorded in
//   plan_text --full          every plan in full
//   plan_text --plan "LABEL"  one plan in full (the label as the summary prints it), for diffing two builds
//
// build_plan only sizes tensors and records launches, so a stand-in handle (ccvpe_max_micro_batch's) is enough: no HIP call is made.
// Every tiled launch's closure is run once with Ctx::probe set, as autotune_plan does: it copies its ConvParams and launches nothing.
// With an unfinalised handle the packed sizes (gemm_n, gemm_kpad, the Winograd and proj flags, composed level 6) are zero or off.
// The capture rule's check: link ccvpe_plan.hip into the program with -Xarch_host -fsanitize=address (the closures are probed
// after build_plan's frame is gone).
#include "ccvpe_internal.h"

#include <cinttypes>

static float g_base[64];   // the fake arena: addresses are formed from it and never read

static void appendf(std::string& s, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    s += buf;
}

struct Flavour { const char* name; void (*set)(ccvpe_handle_s&); };
static const Flavour FLAVOURS[] = {
    {"default", [](ccvpe_handle_s&) {}},
    {"nopad", [](ccvpe_handle_s& h) { h.sw.pad_concat = false; }},
    {"preplate", [](ccvpe_handle_s& h) { h.sw.match_prep_early = false; }},
    {"debug", [](ccvpe_handle_s& h) { h.debug = true; }},
    {"graph", [](ccvpe_handle_s& h) { h.sw.graph_mode = 1; }},
    {"bf16x3", [](ccvpe_handle_s& h) { h.cfg.reserved[0] = 1; }},
    {"noreuse_circ", [](ccvpe_handle_s& h) { h.sw.no_reuse = true; h.cfg.circular_padding = 1; }},
};
struct Form { const char* name; bool pose, topk, summary, heading, hprior, credible; };
static const Form FORMS[] = {
    {"full", false, false, false, false, false, false},     {"pose", true, false, false, false, false, false},
    {"topk", true, true, false, false, false, false},       {"summary", true, false, true, false, false, false},
    {"heading", true, false, false, true, false, false},    {"heading+summary", true, false, true, true, false, false},
    {"hprior", true, false, false, true, true, false},      {"credible", true, false, false, false, false, true},
};
static const int GRD[4][2] = {{320, 640}, {320, 640}, {256, 1024}, {154, 231}};

static std::string plan_text(ccvpe_handle_s& h, const PlanKey& key, int& rc, size_t& nops, size_t& ntensors, size_t& total, size_t& tickets) {
    Plan pl;
    std::string s;
    ccvpe_err().clear();
    rc = build_plan(&h, pl, key);
    nops = pl.ops.size(); ntensors = pl.size.size(); total = pl.total; tickets = pl.ticket_words;
    if (rc != 0) {
        appendf(s, "rc %d: %s\n", rc, ccvpe_err().c_str());
        nops = ntensors = total = tickets = 0;
        return s;
    }
    appendf(s, "rc %d tensors %zu total %zu ticket_words %zu two_streams %d use_graph %d l6_wm %d\n", rc, pl.size.size(), pl.total, pl.ticket_words,
            (int)pl.two_streams, (int)pl.use_graph, pl.l6_wm);
    Ctx c;
    c.arena = g_base; c.off = &pl.off; c.grd = g_base; c.sat = g_base; c.cache_in = g_base; c.cache_out = g_base; c.grd_cache_in = g_base;
    c.tickets = reinterpret_cast<unsigned*>(g_base);
    for (size_t i = 0; i < pl.ops.size(); ++i) {
        const Op& op = pl.ops[i];
        appendf(s, "op %zu %s s%d wait", i, op.name.c_str(), op.stream);
        for (int w : op.wait_on) appendf(s, " %d", w);
        appendf(s, " signal %d flops %.17g bytes %.17g gemm %d %d %d cin %d flags %d%d%d%d%d%d tile %d uses", (int)op.signal, op.flops, op.bytes, op.gemm_m,
                op.gemm_n, op.gemm_kpad, op.conv_cin, (int)op.bf16x3_only, (int)op.wino_ok, (int)op.wino4_ok, (int)op.wino4x_ok, (int)op.is_pw,
                (int)op.proj_ok, op.tile ? 1 : 0);
        for (int id : op.uses) appendf(s, " %d[%zu@%zu]", id, pl.size[id], pl.off[id]);
        s += "\n";
        if (!op.tile) continue;
        ConvParams q{};
        pl.set_scratch(c, op.stream);
        c.probe = &q;
        op.fn(c);
        c.probe = nullptr;
        appendf(s, "  conv in %td ld %d split %d geom %d %d %d %d -> %d %d k %d %d s %d pad %d %d N %d M %d act %d mode %d dcout %d gate %d resid %d ndst %d", q.in - g_base,
                q.in_ld, q.in_split, q.B, q.H, q.W, q.Cin, q.OH, q.OW, q.KH, q.KW, q.stride, q.pad_t, q.pad_l, q.N, q.M, q.act, q.mode, q.deconv_cout,
                q.gate ? 1 : 0, q.resid ? 1 : 0, q.ndst);
        for (int d = 0; d < q.ndst && d < 3; ++d) appendf(s, " (%td %d %d)", q.dst[d].ptr - g_base, q.dst[d].ld, q.dst[d].coff);
        appendf(s, " tick %zu\n", c.conv_tick_off);
    }
    for (const auto& kv : pl.taps) appendf(s, "tap %s %d %d %d\n", kv.first.c_str(), kv.second.t.id, kv.second.coff, kv.second.C);
    s += "issue_order";
    for (int i : pl.issue_order) appendf(s, " %d", i);
    s += "\n";
    return s;
}

static uint64_t fnv1a(const std::string& s) {
    uint64_t x = 1469598103934665603ull;
    for (unsigned char ch : s) { x ^= ch; x *= 1099511628211ull; }
    return x;
}

int main(int argc, char** argv) {
    const bool full = argc > 1 && std::strcmp(argv[1], "--full") == 0;
    const bool compact = argc > 1 && std::strcmp(argv[1], "--compact") == 0;
    const char* one = argc > 2 && std::strcmp(argv[1], "--plan") == 0 ? argv[2] : nullptr;
    bool found = false;
    const Switches env = read_switches();
    for (int v = 0; v < 4; ++v)
    for (int two = 0; two < 2; ++two)
    for (int fuse = 0; fuse < 2; ++fuse)
    for (const Flavour& fl : FLAVOURS) {
        auto h = std::make_unique<ccvpe_handle_s>();   // the stand-in handle of max_micro_batch (ccvpe_api.hip)
        h->cfg.variant = v; h->cfg.ori_noise = 36.f; h->cfg.micro_batch = 1;
        h->vs = make_variant(v);
        h->sw = env;
        h->sw.two_streams = two != 0; h->sw.fuse_level1 = fuse != 0;
        const int n = (int)(h->cfg.ori_noise / 18.f);
        for (int k = 0; k < 6; ++k) h->rolls[k] = (v == CCVPE_VARIANT_VIGOR_ORI_PRIOR && k > 0) ? 2 * n + 1 : h->vs.n_rolls;
        fl.set(*h);
        for (int B : {1, 3}) {
        if (compact) std::printf("v%d streams%d fuse%d %s B%d |", v, two + 1, fuse, fl.name, B);
        for (int mode = 0; mode < 5; ++mode)
        for (const Form& f : FORMS) {
            char label[160];
            std::snprintf(label, sizeof label, "v%d streams%d fuse%d %s B%d mode%d %s", v, two + 1, fuse, fl.name, B, mode, f.name);
            if (one && std::strcmp(one, label) != 0) continue;
            PlanKey key;
            key.B = B; key.gh = GRD[v][0]; key.gw = GRD[v][1]; key.mode = mode;
            key.pose = f.pose; key.topk = f.topk; key.summary = f.summary; key.heading = f.heading; key.hprior = f.hprior; key.credible = f.credible;
            int rc;
            size_t nops, ntensors, total, tickets;
            const std::string text = plan_text(*h, key, rc, nops, ntensors, total, tickets);
            found = true;
            if (full || one) std::printf("== %s\n%s", label, text.c_str());
            else if (compact) std::printf(" %08x", (unsigned)(fnv1a(text) & 0xffffffffu));
            else std::printf("%s | %d %zu %zu %zu %zu %016" PRIx64 "\n", label, rc, nops, ntensors, total, tickets, fnv1a(text));
        }
        if (compact) std::printf("\n");
        }
    }
    if (one && !found) { std::fprintf(stderr, "no plan is labelled \"%s\"\n", one); return 2; }
    return 0;
}
