// The execution plan of libccvpe_hip.so: CVM_*.forward (reference models.py:150-343, 448-652, 752-950, 1051-1244) restated
// as a static list of kernel launches over NHWC tensors; concatenations are channel-offset writes into pre-allocated
// buffers, the encoder taps are written by the producing GEMM's epilogue.
#include "ccvpe_internal.h"

// ------------------------------------------------------------------------------------------------
// roll shifts (spec.py roll_shifts / full_roll_shifts; models.py:192-193, 489-491, 1094)
// ------------------------------------------------------------------------------------------------
static int window_offset(const VariantSpec& vs, int level, int L) {
    const int C = vs.match_ch[level];
    return vs.centre ? (int)((double)C / 2 - (double)L / 2) : 0;
}
static int mod(int a, int m) { int r = a % m; return r < 0 ? r + m : r; }

// ------------------------------------------------------------------------------------------------
// plan construction
// ------------------------------------------------------------------------------------------------
ConvParams conv_params(const PackedConv& pc, const float* in, int in_ld, int B, int H, int W, int OH, int OW,
                              int stride, int pad_t, int pad_l, int act) {
    ConvParams p{};
    p.in = in; p.in_ld = in_ld; p.B = B; p.H = H; p.W = W; p.Cin = pc.cinp; p.OH = OH; p.OW = OW;
    p.KH = pc.KH; p.KW = pc.KW; p.stride = stride; p.pad_t = pad_t; p.pad_l = pad_l;
    p.wpk = pc.w; p.w_hi = pc.w_hi; p.w_lo = pc.w_lo; p.Kpad = pc.Kpad; p.Npad = round_up(pc.N, conv_igemm_npad()); p.nchunks = pc.nchunks; p.bias = pc.bias; p.N = pc.N; p.act = act;
    p.gate = nullptr; p.resid = nullptr; p.resid_ld = 0; p.ndst = 0; p.mode = MODE_CONV; p.deconv_cout = 0;
    p.M = B * OH * OW;
    p.in_bytes = (unsigned)((size_t)B * H * W * in_ld * sizeof(float));
    p.gate_bytes = (unsigned)((size_t)B * pc.cinp * sizeof(float));
    p.w_plane_bytes = (unsigned)((size_t)p.Npad * pc.Kpad * sizeof(unsigned short));
    p.wino_w = pc.wino; p.wino_n16 = pc.wino_n16; p.wino_bytes = (unsigned)pc.wino_bytes;
    p.wino4_w = pc.wino4; p.wino4_bytes = (unsigned)pc.wino4_bytes;
    p.wino4x_w = pc.wino4x; p.wino4x_bytes = (unsigned)pc.wino4x_bytes; p.wino4x_cfg = pc.wino4x_cfg;
    p.proj_w = pc.proj; p.proj_bytes = (unsigned)pc.proj_bytes;
    return p;
}

struct EncOut { Tensor vol; Tensor tap[16]; };

// dsts for tap blocks: concat tensors the project GEMM also writes into (level index 0..4 -> block TAP_BLOCK[i])
struct TapDst { Tensor t[2]; int coff[2]; int n = 0; };

static void plan_encoder(ccvpe_handle_s* h, Plan& pl, const EncoderW& ew, bool is_grd, int B, int H, int W, bool circular,
                         const TapDst* tapdst, EncOut& out, const std::string& tag) {
    int lo, hi;
    static_pad(3, 2, lo, hi);
    int ch = conv_out(H, 3, 2), cw = conv_out(W, 3, 2);
    // stem + the depthwise conv of block 0 in one launch (block 0 has no expand conv; kernels_encoder.hip): the half-resolution 32-channel
    // stem output never reaches HBM.  CCVPE_STEM_DW=0: two launches
    // A circular encoder on an odd image width keeps the two launches too: the fused kernel wraps the halo columns of the stem output by
    // wrapping the INPUT column, which is the same pixel only where W = 2 OW (213 -> 106: stem column -1 is 105 = input 210..212, not 211..213)
    const bool stem_dw = h->sw.stem_dw && B0[0].e == 1 && B0[0].k == 3 && B0[0].s == 1 && B0[0].cin == 32 && !(circular && (W & 1)) &&
                         (size_t)B * 3 * H * W * sizeof(float) < ((size_t)1 << 31);   // (the kernel addresses its input through one 32-bit buffer descriptor)
    StemParams stem_sp{};
    stem_sp.B = B; stem_sp.H = H; stem_sp.W = W; stem_sp.OH = ch; stem_sp.OW = cw; stem_sp.pad_t = lo; stem_sp.pad_l = lo; stem_sp.circular = circular;
    stem_sp.w = ew.stem_w; stem_sp.bias = ew.stem_b;
    Tensor cur = stem_dw ? Tensor{} : pl.alloc(B, ch, cw, 32);
    if (!stem_dw) {
        const StemParams sp = stem_sp;
        Tensor o = cur;
        pl.add(tag + ".stem", {o}, [sp, o, is_grd](const Ctx& c) {
            StemParams q = sp; q.in = is_grd ? c.grd : c.sat; q.out = c.ptr(o);
            launch_stem(q, c.stream);
        }, 2.0 * B * ch * cw * 32 * 27, 4.0 * B * (3.0 * H * W + 32.0 * ch * cw));
    }
    for (int i = 0; i < 16; ++i) {
        const BlockSpec& b = B0[i];
        const BlockW& bw = ew.blk[i];
        const int mid = b.cin * b.e;
        const std::string bn = tag + ".b" + std::to_string(i);
        Tensor xin = cur;
        Tensor e = xin;
        static_pad(b.k, b.s, lo, hi);
        const int oh = conv_out(ch, b.k, b.s), ow = conv_out(cw, b.k, b.s);
        MbFrontParams mp{};
        mp.B = B; mp.H = ch; mp.W = cw; mp.Cin = b.cin; mp.cinp = bw.exp_cinp; mp.mid = mid;
        mp.we = bw.exp_lin; mp.be = bw.expand.bias; mp.wd = bw.dw_w; mp.bd = bw.dw_b;
        mp.k = b.k; mp.s = b.s; mp.pad_t = lo; mp.pad_l = lo; mp.circular = circular; mp.OH = oh; mp.OW = ow;
        // latency plans: the work items a front may spread to = this encoder's share of the 256 CUs - the other encoder's fronts run beside
        // it on the other stream (both at 128: 1.20 ms per VIGOR frame, both at 256: 1.25; the aerial encoder is the longer chain).  The aerial
        // encoder takes 144 whatever it runs beside (its launches must not depend on the ground image: the aerial-only plan of
        // ccvpe_encode_aerial returns the bits of the full forward), the ground encoder its share by input pixels against a 512 x 512 tile.
        {
            const double share = (double)H * W / ((double)H * W + (double)CCVPE_SAT_HW * CCVPE_SAT_HW);
            const int dflt = is_grd ? std::max(64, std::min(128, (int)(256.0 * share / 16.0 + 0.5) * 16)) : 144;
            mp.spread = h->sw.front_spread.value_or(dflt);
        }
        // small-spatial blocks: the whole expanded image of 16 channels lives in LDS (kernels_mbimg.hip); CCVPE_FUSE_MBCONV=0 / CCVPE_MBCONV_IMAGE=0 turn it off
        const bool image = b.e != 1 && bw.exp_lin != nullptr && h->sw.fuse_mbconv != 0 && h->sw.mbconv_image && mbconv_image_supported(mp);
        const bool fused = image || (b.e != 1 && bw.exp_lin != nullptr && mbconv_front_supported(b.k, b.s, b.cin, mid) &&
                           (h->sw.fuse_mbconv == 2 || (h->sw.fuse_mbconv == 1 && mbconv_front_profitable(b.k))));
        Tensor d = pl.alloc(B, oh, ow, mid);
        const bool with_stem = stem_dw && i == 0;
        // Squeeze-excite by ticket (round 4, ticket.h; model.py:113-118): the front kernel's last-arriving workgroup of a sample reduces the
        // pooling partials and computes the gates - no launch of its own.  CCVPE_SE_TICKET=0 keeps the separate launches; kernels that
        // take no ticket (plain depthwise, the workgroup form of the tile kernel) keep them too.
        const bool ticket_on = h->sw.se_ticket && mid <= 1152 && bw.sq <= 64;
        const int trows = !ticket_on ? 0 : with_stem ? stem_dw_tiles(oh, ow) : image ? mbconv_image_ticket_rows(mp) : fused ? mbconv_front_ticket_rows(mp) : 0;
        // Opt-in (CCVPE_SE_PROLOGUE=1; measured, not the default): latency plans (batch <= 4, blocks of <= 4096 rows) without a ticket either -
        // the image-resident front leaves its per-item squeeze rows and the latency-form project GEMM computes the gates in its prologue,
        // every wave those of its own K slice (kernels_proj.hip).  The front kernel loses its ~10 us combining step (block 12: 24.8 -> 15.5 us)
        // but the project GEMM gains as much (9.7 -> 20.9 us: rows -> squeezed vector -> gates is the same chain of dependent round trips,
        // now in front of its MFMAs, and its 128-register waves cannot keep all four kinds of requests in flight at once): 1.41 against
        // 1.28 ms per batch-1 frame.
        bool sep = false;
        if (trows > 0 && image && bw.project.proj != nullptr && h->cfg.reserved[0] == 0 && h->sw.se_prologue) {
            ConvParams q = conv_params(bw.project, nullptr, mid, B, oh, ow, oh, ow, 1, 0, 0, ACT_NONE);
            q.M = B * oh * ow;
            q.se_rows = reinterpret_cast<const float*>(1); q.se_nrows = trows * (mid / 16); q.se_sq = bw.sq;
            sep = conv_proj_supported(q, 101);
        }
        const bool ticket = trows > 0 && !sep;
        const int S = ticket ? trows : with_stem ? stem_dw_tiles(oh, ow) : image ? mbconv_image_strips(mp) : fused ? mbconv_front_tiles(b.k, b.s, oh, ow) : depthwise_strip_lanes(B, oh, ow, mid, b.k, b.s);
        Tensor pool = pl.alloc(B, 1, S, mid);
        Tensor gate = pl.alloc(B, 1, 1, mid);
        SeTicket se{};
        size_t tick_off = 0;
        if (sep) {   // rows only: SeTicket::counter stays null, sqpart set (mbconv_image_kernel: no ticket, no combining step)
            se.per_sample = trows * (mid / 16);
            se.S = trows; se.C = mid; se.SQ = bw.sq; se.inv_hw = 1.f / (float)(oh * ow);
            se.w1 = bw.se_w1;
        }
        if (ticket) {
            tick_off = pl.alloc_tickets((size_t)B);
            se.per_sample = with_stem ? S : image ? S * (mid / 16) : S * mbconv_front_ticket_split(mp);   // tiles | (strip, 16-channel chunk) items | workgroups of a sample
            se.S = S; se.C = mid; se.SQ = bw.sq; se.inv_hw = 1.f / (float)(oh * ow);
            se.w1 = bw.se_w1; se.b1 = bw.se_b1; se.w2 = bw.se_w2; se.b2 = bw.se_b2;
            se.spec = (long long)B * se.per_sample <= 256 ? 1 : 0;   // latency plans: one workgroup per item, the chip not even filled once
        }
        // the image-resident kernel runs the squeeze conv per item (one row of SQ floats each); the others hand over pooling partial rows
        const bool parts = (ticket && image) || sep;
        Tensor sqp = parts ? pl.alloc(B, 1, se.per_sample, bw.sq) : Tensor{};
        auto fill_se = [=](const Ctx& c) {
            SeTicket t = se;
            if (ticket) { t.counter = c.tickets + tick_off; t.pool = c.ptr(pool); t.gate = c.ptr(gate); }
            if (parts) t.sqpart = c.ptr(sqp);
            return t;
        };
        const double se_flops = ticket ? 4.0 * B * mid * bw.sq : 0.0;
        if (with_stem) {
            StemDwParams sd{};
            sd.st = stem_sp; sd.wd = bw.dw_w; sd.bd = bw.dw_b;
            std::vector<Tensor> uses = {d, pool};
            if (ticket) uses.push_back(gate);
            pl.add(tag + ".stem_b0dw", uses, [=](const Ctx& c) {
                StemDwParams q = sd; q.st.in = is_grd ? c.grd : c.sat; q.out = c.ptr(d); q.pool_partial = c.ptr(pool); q.se = fill_se(c);
                launch_stem_dw(q, c.stream);
            }, 2.0 * B * ch * cw * 32 * 27 + 2.0 * B * oh * ow * mid * 9 + se_flops, 4.0 * B * (3.0 * H * W + 32.0 * oh * ow));
        } else if (fused) {
            std::vector<Tensor> uses = {xin, d, pool};
            if (ticket) uses.push_back(gate);
            if (parts) uses.push_back(sqp);
            (void)sep;
            pl.add(bn + ".expand_dw", uses, [=](const Ctx& c) {
                MbFrontParams q = mp; q.x = c.ptr(xin); q.out = c.ptr(d); q.pool = c.ptr(pool); q.se = fill_se(c);
                if (image) launch_mbconv_image(q, c.stream); else launch_mbconv_front(q, c.stream);
            }, 2.0 * B * ch * cw * b.cin * mid + 2.0 * B * oh * ow * mid * b.k * b.k + se_flops, 4.0 * B * ((double)ch * cw * b.cin + (double)oh * ow * mid));
        } else {
        if (b.e != 1) {
            e = pl.alloc(B, ch, cw, mid);
            const PackedConv* pc = &bw.expand;
            const int hh = ch, ww = cw;
            pl.add_conv(bn + ".expand", {xin, e}, B * hh * ww, pc->N, pc->Kpad, [=](const Ctx& c, int tile) {
                ConvParams p = conv_params(*pc, c.ptr(xin), xin.C, B, hh, ww, hh, ww, 1, 0, 0, ACT_SWISH);
                p.dst[0] = {c.ptr(e), mid, 0}; p.ndst = 1;
                c.launch_conv(p, tile);
            }, 2.0 * B * ch * cw * b.cin * mid, 4.0 * B * ch * cw * (b.cin + mid));
            pl.ops.back().is_pw = true;
        }
        {
            DwParams dp{};
            dp.B = B; dp.H = ch; dp.W = cw; dp.C = mid; dp.OH = oh; dp.OW = ow; dp.k = b.k; dp.stride = b.s;
            dp.pad_t = lo; dp.pad_l = lo; dp.circular = circular; dp.w = bw.dw_w; dp.bias = bw.dw_b; dp.S = S;
            pl.add(bn + ".dw", {e, d, pool}, [=](const Ctx& c) {
                DwParams q = dp; q.in = c.ptr(e); q.out = c.ptr(d); q.pool_partial = c.ptr(pool);
                launch_depthwise(q, c.stream);
            }, 2.0 * B * oh * ow * mid * b.k * b.k, 4.0 * B * mid * ((double)ch * cw + (double)oh * ow));
        }
        }
        const int SC = std::max(1, std::min(16, S / 32));
        Tensor pooled = pl.alloc(B, 1, SC, mid);
        Tensor sqt = pl.alloc(B, 1, 1, 64);
        if (!ticket && !sep) {
            SeParams sp{};
            sp.B = B; sp.S = S; sp.C = mid; sp.SQ = bw.sq; sp.inv_hw = 1.f / (float)(oh * ow); sp.SC = SC;
            sp.w1 = bw.se_w1; sp.b1 = bw.se_b1; sp.w2 = bw.se_w2; sp.b2 = bw.se_b2;
            pl.add(bn + ".se", {pool, gate, pooled, sqt}, [=](const Ctx& c) {
                SeParams q = sp; q.pool_partial = c.ptr(pool); q.gate = c.ptr(gate); q.pooled = c.ptr(pooled); q.sq = c.ptr(sqt);
                launch_se(q, c.stream);
            }, 4.0 * B * mid * bw.sq, 4.0 * B * S * mid);
        }
        Tensor o = pl.alloc(B, oh, ow, b.cout);
        {
            const PackedConv* pc = &bw.project;
            const bool skip = (b.s == 1 && b.cin == b.cout);
            TapDst td;
            if (tapdst) for (int t = 0; t < 5; ++t) if (TAP_BLOCK[t] == i) td = tapdst[t];
            std::vector<Tensor> uses = {d, sep ? sqp : gate, o};
            if (skip) uses.push_back(xin);
            for (int t = 0; t < td.n; ++t) uses.push_back(td.t[t]);
            const int se_nrows = se.per_sample, se_sq = bw.sq;
            const float se_inv = se.inv_hw;
            const float *se_b1 = bw.se_b1, *se_w2 = bw.se_w2, *se_b2 = bw.se_b2;
            pl.add_conv(bn + (sep ? ".se_project" : ".project"), uses, B * oh * ow, pc->N, pc->Kpad, [=](const Ctx& c, int tile) {
                ConvParams p = conv_params(*pc, c.ptr(d), mid, B, oh, ow, oh, ow, 1, 0, 0, ACT_NONE);
                if (sep) {
                    p.se_rows = c.ptr(sqp); p.se_nrows = se_nrows; p.se_sq = se_sq; p.se_inv_hw = se_inv; p.se_b1 = se_b1; p.se_w2 = se_w2; p.se_b2 = se_b2;
                    tile = conv_proj_lat_tile();   // the only kernel that computes the gates itself
                } else {
                    p.gate = c.ptr(gate);
                }
                if (skip) { p.resid = c.ptr(xin); p.resid_ld = xin.C; }
                p.dst[0] = {c.ptr(o), o.C, 0}; p.ndst = 1;
                for (int t = 0; t < td.n; ++t) p.dst[p.ndst++] = c.dst(td.t[t], td.coff[t]);
                c.launch_conv(p, tile);
            }, 2.0 * B * oh * ow * mid * b.cout + (sep ? 4.0 * B * mid * bw.sq : 0.0), 4.0 * B * oh * ow * (mid + b.cout * (1 + td.n)));
            pl.ops.back().is_pw = true;
            pl.ops.back().proj_ok = pc->proj != nullptr && h->cfg.reserved[0] == 0;
            if (sep) pl.ops.back().tile.reset();   // not a tuning candidate: one kernel serves it (the launch above names its tile)
        }
        out.tap[i] = o;
        pl.taps[tag + "_block" + std::to_string(i)] = {o, 0, o.C};
        cur = o; ch = oh; cw = ow;
    }
    Tensor vol = pl.alloc(B, ch, cw, 1280);
    {
        const PackedConv* pc = &ew.head;
        Tensor x = cur;
        const int hh = ch, ww = cw;
        pl.add_conv(tag + ".head", {x, vol}, B * hh * ww, pc->N, pc->Kpad, [=](const Ctx& c, int tile) {
            ConvParams p = conv_params(*pc, c.ptr(x), x.C, B, hh, ww, hh, ww, 1, 0, 0, ACT_SWISH);
            p.dst[0] = {c.ptr(vol), 1280, 0}; p.ndst = 1;
            c.launch_conv(p, tile);
        }, 2.0 * B * ch * cw * 320 * 1280, 4.0 * B * ch * cw * 1600);
        pl.ops.back().is_pw = true;
    }
    out.vol = vol;
    pl.taps[tag + "_volume"] = {vol, 0, 1280};
}

// Aerial cache: everything the decoders need from the aerial image, NHWC fp32, batch-major:
// [descriptor map B x 8x8 x D | block15 B x 16^2 x 320 | block10 B x 32^2 x 112 | block4 B x 64^2 x 40 |
//  block2 B x 128^2 x 24 | block0 B x 256^2 x 16]
static const int TAP_HW[5] = {256, 1024, 4096, 16384, 65536};
static const int TAP_C[5] = {320, 112, 40, 24, 16};
size_t cache_layout(const VariantSpec& vs, int B, size_t off[6]) {
    size_t o = 0;
    off[0] = o; o += (size_t)B * 64 * vs.sat_desc;
    for (int t = 0; t < 5; ++t) { off[t + 1] = o; o += (size_t)B * TAP_HW[t] * TAP_C[t]; }
    return o;
}

static int build_aerial_plan(ccvpe_handle_s* h, Plan& pl, int B);
static int build_ground_plan(ccvpe_handle_s* h, Plan& pl, int B, int gh, int gw);
extern "C" int ccvpe_max_micro_batch(int32_t variant, float ori_noise, int32_t grd_h, int32_t grd_w);

// Geometry of the ground feature volume (fh x fw) and the per-level descriptor lengths L[k] of a gh x gw ground image, or EINVAL for a
// size the reference itself cannot run: an image some layer's kernel does not fit into (widths below 32: torch refuses a kernel larger
// than its padded input), and - circular encoders - a layer narrower than its padding (widths below 64: the late 5x5 blocks are one
// pixel wide under a padding of 2, torch's circular pad refuses to wrap more than once, and the kernels wrap a column index once).
static int grd_geometry(const VariantSpec& vs, bool circular, int gh, int gw, int& fh, int& fw, int L[6]) {
    if (gh <= 0 || gw <= 0) return ccvpe_fail(CCVPE_EINVAL, "ground image size %d x %d is not positive", gh, gw);
    fh = gh; fw = gw;
    for (int i = -1; i < 16; ++i) {   // the stem (3x3, stride 2), then the 16 blocks' depthwise convs
        const int k = i < 0 ? 3 : B0[i].k, s = i < 0 ? 2 : B0[i].s;
        int lo, hi;
        static_pad(k, s, lo, hi);
        const std::string layer = i < 0 ? "the stem" : "block " + std::to_string(i);
        if (fh + lo + hi < k || fw + lo + hi < k)
            return ccvpe_fail(CCVPE_EINVAL, "ground image %d x %d is too small: it reaches the %d x %d kernel of %s as %d x %d", gh, gw, k, k,
                              layer.c_str(), fh, fw);
        if (circular && fw < std::max(lo, hi))
            return ccvpe_fail(CCVPE_EINVAL, "ground image %d x %d is too narrow for circular padding: %s pads %d columns around a width of %d "
                              "(the padding would wrap more than once)", gh, gw, layer.c_str(), std::max(lo, hi), fw);
        fh = conv_out(fh, k, s); fw = conv_out(fw, k, s);
    }
    if (fh != vs.feat_h)
        return ccvpe_fail(CCVPE_EINVAL, "ground image %dx%d gives a %d-row feature volume, the descriptor heads expect %d rows", gh, gw, fh, vs.feat_h);
    for (int k = 0; k < 6; ++k) {
        L[k] = fw * vs.head_ch[k];
        if (L[k] > vs.match_ch[k])
            return ccvpe_fail(CCVPE_EINVAL, "descriptor length %d exceeds aerial channels %d at level %d", L[k], vs.match_ch[k], k + 1);
    }
    return 0;
}

// Ground cache (ccvpe_encode_ground): the descriptor vector of each query, [B][Ltot] fp32, Ltot = sum of round_up(L_k, 4) - the
// layout of the plans' `desc` tensor, level k at float offset sum_{j<k} round_up(L_j, 4).
int ground_desc_floats(const ccvpe_handle_s* h, int gh, int gw) {
    int fh, fw, L[6];
    if (int rc = grd_geometry(h->vs, h->cfg.circular_padding != 0, gh, gw, fh, fw, L)) return rc;
    int ltot = 0;
    for (int k = 0; k < 6; ++k) ltot += round_up(L[k], 4);
    return ltot;
}

// grd.heads + grd.desc: the ground descriptor heads over the encoder volume `vol` into the returned `desc` tensor ([B][ltot]), or -
// to_cache - into the caller's ground cache (Ctx::cache_out).  The same launches, names and shapes in the full, cached and ground-only plans.
static Tensor plan_grd_desc(ccvpe_handle_s* h, Plan& pl, int B, int fh, int fw, Tensor vol, bool to_cache) {
    const VariantSpec& vs = h->vs;
    int ntot = 0, ltot = 0, hoff[6], loff[6];
    for (int k = 0; k < 6; ++k) { hoff[k] = ntot; ntot += vs.head_ch[k]; loff[k] = ltot; ltot += round_up(fw * vs.head_ch[k], 4); }
    Tensor ghead = pl.alloc(B, fh, fw, ntot);
    Tensor desc = to_cache ? Tensor{} : pl.alloc(B, 1, 1, ltot);
    const PackedConv* pc = &h->grd_heads;
    Tensor x = vol;
    pl.add_conv("grd.heads", {x, ghead}, B * fh * fw, pc->N, pc->Kpad, [=](const Ctx& c, int tile) {
        ConvParams p = conv_params(*pc, c.ptr(x), 1280, B, fh, fw, fh, fw, 1, 0, 0, ACT_NONE);
        p.dst[0] = {c.ptr(ghead), ntot, 0}; p.ndst = 1;
        c.launch_conv(p, tile);
    }, 2.0 * B * fh * fw * 1280 * ntot, 4.0 * B * fh * fw * (1280 + ntot));
    pl.ops.back().is_pw = true;
    pl.ops.back().proj_ok = pc->proj != nullptr && h->cfg.reserved[0] == 0;
    GrdDescParams gp{};
    gp.B = B; gp.Hf = fh; gp.Wf = fw; gp.Ntot = ntot; gp.nlev = 6; gp.Ltot = ltot;
    for (int k = 0; k < 6; ++k) { gp.c[k] = vs.head_ch[k]; gp.off[k] = hoff[k]; gp.wh[k] = h->grd_wh[k]; gp.b2[k] = h->grd_b2[k]; gp.loff[k] = loff[k]; }
    std::vector<Tensor> uses = {ghead};
    if (!to_cache) uses.push_back(desc);
    pl.add("grd.desc", uses, [=](const Ctx& c) {
        GrdDescParams q = gp; q.y = c.ptr(ghead); q.desc = to_cache ? c.cache_out : c.ptr(desc);
        launch_grd_desc(q, c.stream);
    }, 2.0 * B * fh * fw * ntot, 4.0 * B * fh * fw * ntot);
    return desc;
}

// ------------------------------------------------------------------------------------------------
// The pose tail's four launches (ccvpe_internal.h): the kernel parameters from where the working memory is (w), what the call asks (t)
// and the batch.  The plans below and the logits forms of ccvpe_api.hip issue the tail through these and nothing else.
// ------------------------------------------------------------------------------------------------
void issue_softmax_partial(const TailBuffers& w, const TailCall& t, int B, hipStream_t s) {
    SoftmaxParams p{};
    p.logits = w.logits; p.B = B; p.n = TAIL_HW * TAIL_HW; p.partial = w.partial; p.chunks = TAIL_CHUNKS; p.out = nullptr;
    p.prior = t.log_prior; p.prior_stride = t.prior_stride;
    launch_softmax_partial(p, s);
}

void issue_pose_argmax(const TailBuffers& w, const TailCall& t, int B, hipStream_t s) {
    PoseArgmaxParams p{};
    p.logits = w.logits; p.partial = w.partial; p.B = B; p.n = TAIL_HW * TAIL_HW; p.chunks = TAIL_CHUNKS;
    p.pairs = reinterpret_cast<float*>(w.keys); p.tickets = w.tickets; p.index = w.index; p.rows = t.rows;
    p.stats = t.stats; p.prior = t.log_prior; p.prior_stride = t.prior_stride; p.posterior = t.posterior;
    if (t.summary) { p.summary = t.summary; p.summ_part = w.summ_part; p.summary_r = t.summary_r; }
    launch_pose_argmax(p, s);
}

void issue_topk_peaks(const TailBuffers& w, const TailCall& t, int B, hipStream_t s) {
    TopkParams p{};
    p.heat = nullptr; p.logits = w.logits; p.partial = w.partial; p.B = B; p.k = t.topk_k; p.r = t.topk_r;
    p.keys = reinterpret_cast<unsigned long long*>(w.keys); p.tickets = w.tickets; p.index = w.index; p.rows = t.rows;
    p.prior = t.log_prior; p.prior_stride = t.prior_stride;
    launch_topk_peaks(p, s);
}

void issue_pose_heading(const TailBuffers& w, const TailCall& t, int B, hipStream_t s) {
    HeadingParams p{};
    p.logits = w.logits; p.partial = w.partial; p.prior = t.log_prior; p.prior_stride = t.prior_stride;
    p.ori = w.ori; p.index = w.index; p.B = B; p.nbins = t.heading_bins; p.r = t.heading_r;
    p.part = w.head_part; p.bins = w.bins; p.tickets = w.head_tickets; p.heading = t.heading; p.hist = t.hist;
    launch_heading_reduce(p, s);
}

// Credible regions of the map pose.argmax describes - the logits (+ prior) with the partials of softmax.partial, an
// earlier launch - or, belief set, of a stored map: CRED_PASSES launches and one more with a level map, per CRED_SLICE queries
void issue_pose_credible(const TailBuffers& w, const TailCall& t, const float* belief, int B, hipStream_t s) {
    CredibleParams p{};
    p.belief = belief;
    if (!belief) { p.logits = w.logits; p.partial = w.partial; p.prior = t.log_prior; p.prior_stride = t.prior_stride; }
    p.probe = t.cred_probe; p.B = B; p.n_levels = t.cred_levels;
    for (int j = 0; j < CRED_MAX_LEVELS; ++j) p.level[j] = t.cred_level[j];
    credible_scratch(p, B, w.cred_zero, w.cred_state);
    p.tickets = w.cred_tickets; p.cred = t.cred; p.level_map = t.cred_map;
    launch_credible(p, s);
}

// ------------------------------------------------------------------------------------------------
// Launch descriptions: every launch a plan form may hold is described once, by a free function.  A plan outlives its
// builder, so a launch closure captures tensors, small parameter structs and pointers into the handle BY VALUE - these functions have
// no builder to capture by accident.  The order of their pl.alloc / pl.alloc_tickets / pl.add calls is behaviour (tensor ids,
// workspace offsets, ticket ranges, streams by name prefix, tuning keys by name).
// ------------------------------------------------------------------------------------------------

// Every kernel addresses a tensor with 32-bit byte offsets: the largest tensor of the plan, or of the caller's (io_bytes), reaches 2 GiB
static bool tensor_too_large(Plan& pl, size_t io_bytes) {
    pl.max_tensor_bytes = std::max(pl.max_tensor_bytes, io_bytes);
    return pl.max_tensor_bytes >= ((size_t)1 << 31);
}

// The fused last level's parameters from a decoder's composed weights; the caller adds what is its own (x, out, raw, tile, max_wg)
Level1Params level1_params(const DecoderW& dw, int x_ld, int B, int cout, bool normalize) {
    Level1Params lp{};
    lp.x_ld = x_ld; lp.cx = dw.l1_cx; lp.cxp = dw.l1_cxp; lp.B = B; lp.H = CCVPE_OUT_HW; lp.W = CCVPE_OUT_HW;
    lp.c0 = dw.l1_c0; lp.ng = dw.l1_ng; lp.score = dw.l1_score; lp.wc = dw.l1_wc; lp.ws = dw.l1_ws; lp.bc = dw.l1_bc; lp.wt = dw.l1_wt;
    lp.bt[0] = dw.tail_b[0]; lp.bt[1] = dw.tail_b[1]; lp.cout = cout; lp.normalize = normalize ? 1 : 0;
    return lp;
}

// The eligibility flags of a packed 3x3 layer reading `in` (the tuning key is made from them) ...
static void set_conv3x3_flags(const ccvpe_handle_s* h, Op& op, const PackedConv& pc, const Tensor& in) {
    op.bf16x3_only = in.split;
    op.conv_cin = in.C;
    op.wino_ok = pc.wino != nullptr && !in.split && h->sw.wino && h->cfg.reserved[0] == 0;
    op.wino4_ok = op.wino_ok && pc.wino4 != nullptr;
    op.wino4x_ok = op.wino_ok && pc.wino4x != nullptr;
}
// ... and of the composed level 6's skip layer (`skip` input channels in a tensor of `cin`, N outputs), whose packed forms exist only
// once ensure_level6 has run: what pack_conv will pack for a 3x3 layer of these sizes, by pack_conv's own conditions
static void set_skip6_flags(const ccvpe_handle_s* h, Op& op, int cin, int skip, int N) {
    op.conv_cin = cin;
    op.wino_ok = skip % 8 == 0;
    op.wino4_ok = op.wino_ok && N >= h->sw.wino4_min_n && !h->sw.no_wino4;
    op.wino4x_ok = op.wino_ok && N >= 24 && conv_wino4x_config(N) >= 0 && !h->sw.no_wino4x;
}

// One section of the aerial cache (C channels, hw pixels per sample; at float offset `off` in a cache of B samples, `off1` in a cache
// of one) into d0 and, where d1 is a tensor, d1 as well.  Indexed calls (Ctx::tile_index set) run the same plan with a gather in the
// scatter's place: the cache then holds n_tiles samples, so the section starts at its one-sample offset times n_tiles, and sample b
// reads tile tile_index[b].  The indices go by value in the launch arguments - safe because cached plans are never captured into a
// hipGraph, so every call issues launches with its own arguments.
static void add_cache_read(Plan& pl, const std::string& name, int B, size_t off, size_t off1, int C, int hw, Tensor d0, int coff0, Tensor d1,
                           int coff1, double bytes) {
    const int ndst = d1.id >= 0 ? 2 : 1;
    const long long P = (long long)B * hw;
    std::vector<Tensor> uses = {d0};
    if (ndst == 2) uses.push_back(d1);
    pl.add(name, uses, [=](const Ctx& c) {
        const Dst a = c.dst(d0, coff0), b = ndst == 2 ? c.dst(d1, coff1) : Dst{nullptr, 0, 0, 0, 0};
        if (c.tile_index) launch_gather_channels(c.cache_in + off1 * c.n_tiles, C, hw, c.tile_index, B, a, b, ndst, c.stream);
        else launch_scatter_channels(c.cache_in + off, C, P, a, b, ndst, c.stream);
    }, 0, bytes);
}

// Pair plans: each pair's row of the ground cache [n_queries][ltot] - the gather of the aerial side with one "pixel" per sample
static void add_ground_cache_read(Plan& pl, int B, int ltot, Tensor d) {
    pl.add("grd.cached_desc", {d}, [=](const Ctx& c) {
        launch_gather_channels(c.grd_cache_in, ltot, 1, c.query_index, B, c.dst(d), Dst{nullptr, 0, 0, 0, 0}, 1, c.stream);
    }, 0, 8.0 * B * ltot);
}

// The aerial descriptor map: conv k2 s2 over the 1280 x 16 x 16 volume x, into the workspace tensor dmap or - no tensor - into the
// caller's aerial cache (Ctx::cache_out).  One launch, so one tuning-table entry, for the full plan and the aerial-encode plan.
static void add_descmap(ccvpe_handle_s* h, Plan& pl, int B, Tensor x, Tensor dmap) {
    const PackedConv* pc = &h->sat_desc;
    const int D = h->vs.sat_desc;
    std::vector<Tensor> uses = {x};
    if (dmap.id >= 0) uses.push_back(dmap);
    pl.add_conv("sat.descmap", uses, B * 8 * 8, pc->N, pc->Kpad, [=](const Ctx& c, int tile) {
        ConvParams p = conv_params(*pc, c.ptr(x), 1280, B, 16, 16, 8, 8, 2, 0, 0, ACT_NONE);
        p.dst[0] = {dmap.id >= 0 ? c.ptr(dmap) : c.cache_out, D, 0}; p.ndst = 1;
        c.launch_conv(p, tile);
    }, 2.0 * B * 64 * 5120.0 * D, 4.0 * (B * 256 * 1280.0 + 5120.0 * D));
    pl.ops.back().proj_ok = pc->proj != nullptr && h->cfg.reserved[0] == 0;   // (k2s2: the latency form of kernels_proj.hip only)
}

// Level 6 composed (kernels_level6.hip): the Winograd form (0: the three launches), the sizes of the localisation and
// the orientation decoder's composed launches, and sat_block15's dense tensor [B, 16, 16, 320] - the level-6 concat buffers are then
// never written
struct Level6Form {
    int wm = 0; Level6Params p[2] = {}; Tensor skip15;
    // split form of conv6.2 and of conv6.0's skip half (SPLIT6_* bits; Split6Params, kernels_level6.hip): the sizes per decoder
    int split = 0; Split6Params sb[2] = {}, ss[2] = {};
};

// A 3x3 layer of the 16 x 16 map in split form: transform, the grouped GEMM over 36 positions, inverse transform (+ bias, ReLU) into
// `out` - three launches, tag.{layer}_transform, tag.conv_{layer} (the GEMM keeps the layer's launch name) and tag.{layer}_inverse; `wc`
// and `bias` point into the handle's weights, filled before the plan first runs and read at launch
static void plan_split6(Plan& pl, const Split6Params& sp, float* const* wc, float* const* bias, bool relu, Tensor in, Tensor out, const std::string& tag,
                        const std::string& layer) {
    Tensor V = pl.alloc(36, 1, sp.R, sp.Kc), Mp = pl.alloc(36, 1, sp.R, sp.N);
    pl.add(tag + "." + layer + "_transform", {in, V}, [=](const Ctx& c) {
        Split6Params q = sp; q.x = c.ptr(in); q.v = c.ptr(V);
        launch_split6_transform(q, c.stream);
    }, 0.0, 4.0 * ((double)in.numel() + (double)V.numel()));
    pl.add(tag + ".conv_" + layer, {V, Mp}, [=](const Ctx& c) {
        Split6Params q = sp; q.v = c.ptr(V); q.wc = *wc; q.mp = c.ptr(Mp);
        launch_level6_gemm(split6_gemm_params(q), c.stream);
    }, 2.0 * 36 * sp.R * (double)sp.N * sp.Kc, 4.0 * ((double)V.numel() + 36.0 * sp.Npad * sp.Kc + (double)Mp.numel()));
    pl.ops.back().form = "conv_wino4_split";   // an F(4x4,3x3) layer like the tile it replaces: profile rows (and what reads them) say so
    pl.add(tag + "." + layer + "_inverse", {Mp, out}, [=](const Ctx& c) {
        Split6Params q = sp; q.mp = c.ptr(Mp); q.bias = bias ? *bias : nullptr; q.relu = relu ? 1 : 0; q.out = c.ptr(out);
        launch_split6_inverse(q, c.stream);
    }, 0.0, 4.0 * ((double)Mp.numel() + (double)out.numel()));
}

// Composed level 6 of decoder `dw` into `mid`: transform, grouped GEMM, the skip half as a 3x3 convolution of its own (a tiled
// launch: the tuner picks its tile and split), combine (output transform + skip half + border-case bias + ReLU)
static void plan_level6_composed(ccvpe_handle_s* h, Plan& pl, int B, const Level6Form& l6, const DecoderW& dw, const DecLevel& l, Tensor din, Tensor mid,
                                 const std::string& tag) {
    const int hout = 16;
    const Level6W* w6 = &h->l6[&dw == &h->ori ? 1 : 0];   // filled by ensure_level6 before the plan first runs: read at launch
    const Level6Params lp = l6.p[&dw == &h->ori ? 1 : 0];
    const int G = 4 * level6_positions(l6.wm);
    Tensor V = pl.alloc(G, 1, lp.R, lp.Kc), Mp = pl.alloc(G, 1, lp.R, lp.N), sk = pl.alloc(B, hout, hout, l.mid);
    const Tensor s15 = l6.skip15;
    pl.add(tag + ".l6_transform", {din, V}, [=](const Ctx& c) {
        Level6Params q = lp; q.x = c.ptr(din); q.v = c.ptr(V);
        launch_level6_transform(q, c.stream);
    }, 0.0, 4.0 * ((double)din.numel() + (double)V.numel()));
    pl.add(tag + ".l6_gemm", {V, Mp}, [=](const Ctx& c) {
        Level6Params q = lp; q.v = c.ptr(V); q.wc = w6->wc; q.mp = c.ptr(Mp);
        launch_level6_gemm(q, c.stream);
    }, 2.0 * G * lp.R * (double)lp.N * lp.Kc, 4.0 * ((double)V.numel() + (double)G * lp.Npad * lp.Kc + (double)Mp.numel()));
    if (l6.split & SPLIT6_SKIP) {   // the skip half in split form: no bias, no activation, into the same dense tensor
        Split6Params sp = l6.ss[&dw == &h->ori ? 1 : 0];
        sp.x_ld = s15.C;
        plan_split6(pl, sp, &w6->ws, nullptr, false, s15, sk, tag, "skip");
    } else {
        // the skip layer's GEMM shape is known now (N, 9 taps of l.skip channels)
        const PackedConv* pc = &w6->skip;
        pl.add_conv(tag + ".conv_skip", {s15, sk}, B * hout * hout, lp.N, round_up(9 * l.skip, 32), [=](const Ctx& c, int tile) {
            ConvParams p = conv_params(*pc, c.ptr(s15), s15.C, B, hout, hout, hout, hout, 1, 1, 1, ACT_NONE);
            p.dst[0] = c.dst(sk); p.ndst = 1;
            c.launch_conv(p, tile);
        }, 2.0 * B * hout * hout * 9.0 * s15.C * l.mid, 4.0 * B * hout * hout * ((double)s15.C + l.mid));
        set_skip6_flags(h, pl.ops.back(), s15.C, l.skip, lp.N);
    }
    pl.add(tag + ".l6_combine", {Mp, sk, mid}, [=](const Ctx& c) {
        Level6Params q = lp; q.mp = c.ptr(Mp); q.skip = c.ptr(sk); q.bc = w6->bc; q.out = c.ptr(mid);
        launch_level6_combine(q, c.stream);
    }, 0.0, 4.0 * ((double)Mp.numel() + 2.0 * (double)mid.numel()));
}

// Does the transposed conv of decoder level 6-j run on deconv_k2s2_kernel (CCVPE_DECONV_K2S2)?  fp32 plans whose tensors
// are fp32, of at least DECONV_K2S2_MIN_BATCH samples (level 3: DECONV_K2S2_MIN_BATCH_L3), where the kernel takes the sizes; fills kp (all
// but its pointers).  The live input channels follow from the packed layout, not from the weights' values (no device work here): either
// every channel of the layer, or - a scored level, [score | 7 unused | C] - channel 0 and the channels from 8 on (build_decoder's cmap).
static bool deconv_k2s2_planned(const ccvpe_handle_s* h, int B, int j, const PackedConv& pc, const DecLevel& l, const Tensor& din, const Tensor& cat, int cw,
                                DeconvK2S2Params& kp) {
    if (h->cfg.reserved[0] != 0 || din.split || cat.split || j < 2 || j > 4) return false;   // levels 4 .. 2 (level 1 is fused; levels 6 and 5: the wide tiles)
    const int sw = h->sw.deconv_k2s2 ? *h->sw.deconv_k2s2 : -1;
    if (sw == 0 || (sw < 0 && (j < 3 || B < (j == 3 ? DECONV_K2S2_MIN_BATCH_L3 : DECONV_K2S2_MIN_BATCH)))) return false;   // automatic: levels 3 and 2
    if (pc.N != 4 * cw || pc.cinp <= 0 || pc.cinp > din.C || pc.KH != 1 || pc.KW != 1) return false;
    std::vector<unsigned char> live(pc.cinp, 1);
    if (pc.cinp == l.din + score_pad(1) - 1) { for (int c = 1; c < score_pad(1); ++c) live[c] = 0; }
    else if (pc.cinp != l.din) return false;
    const int hin = 8 << j;
    kp.B = B; kp.H = hin; kp.W = hin; kp.Cin = pc.cinp; kp.in_ld = din.C; kp.Kpad = pc.Kpad;
    kp.ld = cat.C; kp.coff = 0; kp.cw = cw;
    return deconv_k2s2_prepare(kp, live.data());
}

// Decoder level 6-j of decoder `dw`: deconv into the concat buffer `cat` (whose skip half the aerial side wrote), conv_a, conv_b.
// Level 1 (j == 5) returns conv_a's output: its tail conv is the caller's.
static Tensor plan_level(ccvpe_handle_s* h, Plan& pl, int B, const Level6Form& l6, const DecoderW& dw, const DecLevel* lv, int j, Tensor din, Tensor cat,
                         const std::string& tag) {
    const int hin = 8 << j, hout = hin * 2;
    const DecLevel& l = lv[j];
    Tensor mid = pl.alloc(B, hout, hout, l.mid);
    if (j == 0 && l6.wm) {
        plan_level6_composed(h, pl, B, l6, dw, l, din, mid, tag);
    } else {
        const PackedConv* pcd = &dw.deconv[j];
        const int cwd = deconv_width(l, h->sw.pad_concat);
        DeconvK2S2Params kp{};
        const double dflops = 2.0 * B * hin * hin * (double)l.din * 4 * l.dout, dbytes = 4.0 * B * hin * hin * ((double)din.C + 4.0 * l.dout);
        if (deconv_k2s2_planned(h, B, j, *pcd, l, din, cat, cwd, kp)) {
            // the transposed conv on its own kernel (kernels_deconv.hip): the launch's name, tensors, FLOPs and bytes are
            // the tiled launch's; not a registry tile - the tuner and the tuning table do not see it
            pl.add(tag + ".deconv", {din, cat}, [=](const Ctx& c) {
                DeconvK2S2Params q = kp;
                q.x = c.ptr(din); q.wpk = pcd->w; q.bias = pcd->bias; q.out = c.ptr(cat);
                launch_deconv_k2s2(q, c.stream);
            }, dflops, dbytes);
            pl.ops.back().form = "conv_pw_k2s2";
        } else {
            const PackedConv* pc = &dw.deconv[j];
            const int cout = deconv_width(l, h->sw.pad_concat);   // (columns past l.dout: zero weights and biases, written as zeros)
            pl.add_conv(tag + ".deconv", {din, cat}, B * hin * hin, pc->N, pc->Kpad, [=](const Ctx& c, int tile) {
                ConvParams p = conv_params(*pc, c.ptr(din), din.C, B, hin, hin, hin, hin, 1, 0, 0, ACT_NONE);
                p.mode = MODE_DECONV; p.deconv_cout = cout;
                p.dst[0] = c.dst(cat); p.ndst = 1;
                c.launch_conv(p, tile);
            }, 2.0 * B * hin * hin * (double)l.din * 4 * l.dout, 4.0 * B * hin * hin * ((double)din.C + 4.0 * l.dout));
            pl.ops.back().is_pw = !din.split;
            pl.ops.back().proj_ok = pc->proj != nullptr && !din.split && h->cfg.reserved[0] == 0;
        }
        mid.split = cat.split;   // bf16x3 mode: conv_a -> conv_b hand-off stays in split bf16 form
        const PackedConv* pc = &dw.conva[j];
        pl.add_conv(tag + ".conv_a", {cat, mid}, B * hout * hout, pc->N, pc->Kpad, [=](const Ctx& c, int tile) {
            ConvParams p = conv_params(*pc, c.ptr(cat), cat.C, B, hout, hout, hout, hout, 1, 1, 1, ACT_RELU);
            p.in_split = cat.split; p.in_plane_bytes = (unsigned)(cat.numel() * 2);
            p.dst[0] = c.dst(mid); p.ndst = 1;
            c.launch_conv(p, tile);
        }, 2.0 * B * hout * hout * 9.0 * cat.C * l.mid, 4.0 * B * hout * hout * ((double)cat.C + l.mid));
        set_conv3x3_flags(h, pl.ops.back(), *pc, cat);
    }
    if (j == 5) return mid;
    Tensor o = pl.alloc(B, hout, hout, l.out);
    const PackedConv* pc = &dw.convb[j];
    if (j == 0 && l6.wm && (l6.split & SPLIT6_CONV_B)) {   // conv6.2 in split form: + bias, into conv_b's tensor
        const int d = &dw == &h->ori ? 1 : 0;
        plan_split6(pl, l6.sb[d], &h->l6[d].wb, &pc->bias, false, mid, o, tag, "b");
        return o;
    }
    pl.add_conv(tag + ".conv_b", {mid, o}, B * hout * hout, pc->N, pc->Kpad, [=](const Ctx& c, int tile) {
        ConvParams p = conv_params(*pc, c.ptr(mid), mid.C, B, hout, hout, hout, hout, 1, 1, 1, ACT_NONE);
        p.in_split = mid.split; p.in_plane_bytes = (unsigned)(mid.numel() * 2);
        p.dst[0] = {c.ptr(o), o.C, 0}; p.ndst = 1;
        c.launch_conv(p, tile);
    }, 2.0 * B * hout * hout * 9.0 * l.mid * l.out, 4.0 * B * hout * hout * ((double)l.mid + l.out));
    set_conv3x3_flags(h, pl.ops.back(), *pc, mid);
    return o;
}

// The fused last level over the whole field: deconv1 + conv1[0] + ReLU + conv1[2] (+ normalize) in one launch, to the caller's buffer
// or - out_ws a tensor - into the workspace (the logits of a pose plan, the orientation field of a heading plan)
static void plan_level1_fused(ccvpe_handle_s* h, Plan& pl, int B, const DecoderW& dw, Tensor din, int cin_real, int cout, bool is_ori, Tensor raw,
                              const std::string& tag, Tensor out_ws) {
    Level1Params lp = level1_params(dw, din.C, B, cout, is_ori);
    lp.tile = h->sw.l1_tile;
    const bool has_raw = raw.id >= 0;
    std::vector<Tensor> uses = {din};
    if (has_raw) uses.push_back(raw);
    if (out_ws.id >= 0) uses.push_back(out_ws);
    const double px = (double)B * CCVPE_OUT_HW * CCVPE_OUT_HW;
    pl.add(tag + ".fused", uses, [=](const Ctx& c) {
        Level1Params q = lp;
        q.x = c.ptr(din);
        q.out = out_ws.id >= 0 ? c.ptr(out_ws) : is_ori ? c.out.ori : c.out.logits_flattened;
        q.raw = has_raw ? c.ptr(raw) : nullptr;
        launch_level1(q, c.stream);
    }, px / 4 * 2.0 * cin_real * 64 + px * 2.0 * 144 * 16 + px * 2.0 * 144 * cout, 4.0 * (px / 4 * lp.cx + px * cout));
}

// The fused orientation level 1 for one 16 x 16 tile per sample, the one that holds its argmax (ori1.pose), or per hypothesis
// (ori1.topk): a wait on pose.argmax / topk.peaks through `idx`; the launch writes rows[2..4] itself
static void add_level1_peaks(ccvpe_handle_s* h, Plan& pl, int B, Tensor din, Tensor idx, bool topk, double cin_real) {
    const Level1Params lp = level1_params(h->ori, din.C, B, 2, true);
    const double px = (double)B * (topk ? 8 : 1) * 16 * 16;   // (top-K: accounted at K = 8)
    const double flops = px / 4 * 2.0 * cin_real * 64 + px * 2.0 * 144 * 16 + px * 2.0 * 144 * 2, bytes = 4.0 * px / 4 * lp.cx;
    if (topk) pl.add("ori1.topk", {din, idx}, [=](const Ctx& c) {
        Level1Params q = lp;
        q.x = c.ptr(din); q.out = nullptr; q.raw = nullptr;
        launch_level1_topk(q, reinterpret_cast<const int*>(c.ptr(idx)), c.tail.topk_k, c.tail.rows, c.stream);
    }, flops, bytes);
    else pl.add("ori1.pose", {din, idx}, [=](const Ctx& c) {
        Level1Params q = lp;
        q.x = c.ptr(din); q.out = nullptr; q.raw = nullptr;
        launch_level1_pose(q, reinterpret_cast<const int*>(c.ptr(idx)), c.tail.rows, c.stream);
    }, flops, bytes);
}

// The unfused tail conv of decoder `dw` over conv_a's output m (loc1.tail: cout 1; ori1.tail: cout 2, normalised): to the caller's
// buffer or - out_ws a tensor, pose plans - into the workspace; raw: the un-normalised copy of a debug handle's full plan
static void add_tail_conv(Plan& pl, const std::string& name, int B, const DecoderW& dw, int cout, Tensor m, Tensor raw, Tensor out_ws) {
    const float* tw = dw.tail_w;
    const float tb0 = dw.tail_b[0], tb1 = cout == 2 ? dw.tail_b[1] : 0.f;
    std::vector<Tensor> uses = {m};
    if (raw.id >= 0) uses.push_back(raw);
    if (out_ws.id >= 0) uses.push_back(out_ws);
    pl.add(name, uses, [=](const Ctx& c) {
        TailConvParams p{};
        p.in = c.ptr(m); p.B = B; p.H = CCVPE_OUT_HW; p.W = CCVPE_OUT_HW; p.w = tw; p.bias[0] = tb0; p.bias[1] = tb1; p.cout = cout;
        p.normalize = cout == 2 ? 1 : 0; p.out = out_ws.id >= 0 ? c.ptr(out_ws) : cout == 2 ? c.out.ori : c.out.logits_flattened;
        p.raw = raw.id >= 0 ? c.ptr(raw) : nullptr;
        launch_tail_conv(p, c.stream);
    }, 2.0 * B * 262144.0 * (144 * cout), 4.0 * B * 262144.0 * (16 + cout));
}

// A matching level's parameters from the variant: the rolls R with their shifts (spec.py roll_shifts / full_roll_shifts), the rolls that
// take part in the max, and the strides of the two concat buffers it writes.  The caller adds x_ld, B, g_ld and the handle's switches.
static MatchParams match_level_params(const VariantSpec& vs, const ccvpe_config& cfg, int k, int L) {
    MatchParams mp{};
    const int C = vs.match_ch[k], rfull = vs.n_rolls;
    mp.HW = (8 << k) * (8 << k); mp.C = C; mp.L = L;
    const int off = window_offset(vs, k, L);
    const bool prior = cfg.variant == CCVPE_VARIANT_VIGOR_ORI_PRIOR;
    const int n = prior ? (int)(cfg.ori_noise / 18.f) : 0;
    if (k == 0 || !prior) {
        mp.R = rfull;
        for (int r = 0; r < rfull; ++r) mp.shift[r] = mod(off + r * vs.step[k], C);
        mp.inmax = 0;
        if (prior) { for (int i = -n; i <= n; ++i) mp.inmax |= 1u << mod(i, rfull); }
        else mp.inmax = rfull >= 32 ? 0xffffffffu : ((1u << rfull) - 1u);
    } else {
        mp.R = 2 * n + 1;
        for (int r = 0; r < mp.R; ++r) mp.shift[r] = mod(off + (r - n) * vs.step[k], C);
        mp.inmax = (mp.R >= 32) ? 0xffffffffu : ((1u << mp.R) - 1u);
    }
    mp.rpad = score_pad(rfull);
    mp.P = match_pixels_per_block(mp.HW, C);
    mp.cat_max_ld = 8 + C;
    mp.cat_all_ld = mp.rpad + C;
    return mp;
}

// The preparation launch of every matching level (rolled descriptor / Gm, Mk) depends on the ground descriptor only: the six of them are
// moved in front of the first matching level, where the localisation stream otherwise waits for the aerial encoder (batch 1: ~40 us off the
// critical path).  CCVPE_MATCH_PREP_EARLY=0: inside each level's launch as before.
struct MatchPrep {
    std::vector<std::function<MatchParams(const Ctx&)>> fills;
    std::vector<Tensor> uses;
    size_t first_op = (size_t)-1;   // the first matching level's launch: match.prep is rotated in front of it
};

// Matching level k+1 (feeds decoder level 6-k): aerial features xin against the ground descriptor at desc + goff, the maximum and the
// normalised features into lin, the first level's whole score stack into oin6 as well (a tensor at level 1 only).  Pose plans skip the
// matching-score store.  prep: the plan prepares early - the level's parameters join match.prep.
static void add_match(Plan& pl, int k, const MatchParams& mp, bool pose, Tensor xin, Tensor desc, int goff, Tensor lin, Tensor oin6, MatchPrep* prep) {
    const int B = mp.B;
    Tensor ggs = pl.alloc(B, 1, 1, (int)match_scratch_floats(mp.C));
    const bool first = oin6.id >= 0;
    std::vector<Tensor> uses = {xin, desc, lin, ggs};
    if (first) uses.push_back(oin6);
    auto fill = [=](const Ctx& c) {        // the same parameters for the preparation and the main launch: both pick the same form
        MatchParams q = mp;
        q.x = c.ptr(xin); q.g = c.ptr(desc) + goff;
        q.ms = pose ? nullptr : c.out.matching_score[k];
        q.cat_max = c.ptr(lin);
        q.cat_all = first ? c.ptr(oin6) : nullptr;
        q.gg_scratch = c.ptr(ggs);
        return q;
    };
    if (prep) {
        prep->fills.push_back(fill);
        if (prep->uses.empty()) prep->uses.push_back(desc);
        prep->uses.push_back(ggs);
    }
    pl.add("match" + std::to_string(k + 1), uses, [=](const Ctx& c) { launch_match(fill(c), c.stream); },
           4.0 * B * mp.HW * (double)mp.R * mp.L, 4.0 * B * mp.HW * (2.0 * mp.C + mp.R + 8));
}

// The preparation of all levels: ONE launch (kernels_match.hip), moved in front of the first matching level
static void add_match_prep(Plan& pl, const MatchPrep& prep) {
    const size_t n0 = pl.ops.size();
    const auto prep_fills = prep.fills;
    pl.add("match.prep", prep.uses, [prep_fills](const Ctx& c) {
        MatchParams ps[6];
        const int n = (int)std::min<size_t>(prep_fills.size(), 6);
        for (int i = 0; i < n; ++i) ps[i] = prep_fills[i](c);
        launch_match_prep_all(ps, n, c.stream);
    }, 0.0, 0.0);
    std::rotate(pl.ops.begin() + prep.first_op, pl.ops.begin() + n0, pl.ops.end());
}

// Pose plans: the tail's tensors and ticket ranges, and its working memory for a launch context (ids < 0: null).  Filled as the tail's
// launches are added; each launch captures the copy of its moment, so it sees no range or tensor that was added behind it.
struct TailTensors {
    Tensor logits, ori;   // the logits and, heading plans, the whole orientation field in the workspace
    Tensor part, keys;    // the softmax partials (read again by pose.heading); the (max, index) pairs or the top-K keys
    Tensor index;         // [B] argmax (int32), read by the orientation side; top-K: [B][K] (-1: no peak)
    Tensor spart, hpart;  // the float64 hand-offs of the summary and the heading sums
    Tensor cstate;        // the states of pose.credible's passes
    size_t toff = 0, htoff = 0, boff = 0;   // ticket ranges: pose.argmax or topk.peaks, pose.heading, its fixed-point histograms
    size_t ctoff = 0, czoff = 0;            // ... pose.credible and its histograms
    TailBuffers at(const Ctx& c) const {
        auto ptr = [&](const Tensor& t) { return t.id < 0 ? nullptr : c.ptr(t); };
        TailBuffers w;
        w.logits = ptr(logits); w.ori = ptr(ori); w.partial = ptr(part); w.keys = ptr(keys); w.index = reinterpret_cast<int*>(ptr(index));
        w.summ_part = reinterpret_cast<double*>(ptr(spart)); w.head_part = reinterpret_cast<double*>(ptr(hpart));
        w.tickets = c.tickets + toff; w.head_tickets = c.tickets + htoff; w.bins = reinterpret_cast<unsigned long long*>(c.tickets + boff);
        w.cred_tickets = c.tickets + ctoff; w.cred_zero = c.tickets + czoff; w.cred_state = ptr(cstate);
        return w;
    }
};

// What a tail launch is asked: the context's call with the position prior it reads.  A position prior (Ctx::tail.log_prior, ccvpe_*_prior,
// DESIGN.md 4.10) changes no launch: softmax.partial, pose.argmax, topk.peaks and pose.heading read it beside the logits, each call with
// its own pointer and stride.  Heading-prior plans (comb a tensor) read the plan's combined map in the caller's prior's place.
struct TailPrior {
    Tensor comb;
    TailCall call(const Ctx& c) const {
        TailCall t = c.tail;
        if (comb.id >= 0) { t.prior_stride = (long long)CCVPE_OUT_HW * CCVPE_OUT_HW; t.log_prior = c.ptr(comb); }
        return t;
    }
};

// The tail of a pose plan behind the logits in the workspace: the first softmax launch alone, then pose.argmax (argmax and prob from
// recomputed heatmap values) - the [B][5] result rows of ccvpe_postprocess_rows and nothing else.
// Top-K pose plans (ccvpe_localize_topk): topk.peaks in pose.argmax's place (the K best peaks from recomputed heatmap values, DESIGN.md
// 4.7).  K and r come with each call (TailCall::topk_k / topk_r); the workspace is sized for K = 64.
// Credible plans (ccvpe_localize_credible*): pose.credible - the radix select's launches - behind pose.argmax on its
// stream, reading the logits the workspace still holds; the histograms live beside the counters (zero between launches), the passes'
// states in the workspace.
static void add_pose_tail(Plan& pl, int B, Tensor logits_ws, const TailPrior prior, TailTensors& tt) {
    const bool topk = pl.key.topk, summ = pl.key.summary, hprior = prior.comb.id >= 0;
    tt.logits = logits_ws;
    tt.part = pl.alloc(B, 1, TAIL_CHUNKS, 2); tt.keys = pl.alloc(B, 1, TAIL_CHUNKS, topk ? 2 * TOPK_MAX_K : 2);
    tt.index = pl.alloc(B, 1, 1, topk ? TOPK_MAX_K : 1);
    // summary plans: the chunks' float64 sums, B x 64 x 8 doubles (tensors start on 256-byte granules); no other
    // plan allocates it, so theirs keep their workspace
    static_assert(sizeof(double) == 2 * sizeof(float), "the hand-off is allocated in floats");
    if (summ) tt.spart = pl.alloc(B, 1, TAIL_CHUNKS, 2 * SUMMARY_PART);
    std::vector<Tensor> sm_uses = {tt.logits, tt.part};
    if (hprior) sm_uses.push_back(prior.comb);
    const TailTensors w = tt;
    pl.add("softmax.partial", sm_uses, [=](const Ctx& c) { issue_softmax_partial(w.at(c), prior.call(c), B, c.stream); }, 0, 4.0 * B * 262144.0);
    tt.toff = pl.alloc_tickets((size_t)B);
    const TailTensors wt = tt;
    if (topk) pl.add("topk.peaks", {tt.logits, tt.part, tt.keys, tt.index}, [=](const Ctx& c) { issue_topk_peaks(wt.at(c), prior.call(c), B, c.stream); },
                     0, 4.0 * B * 262144.0);
    std::vector<Tensor> am_uses = {tt.logits, tt.part, tt.keys, tt.index};
    if (summ) am_uses.push_back(tt.spart);
    if (hprior) am_uses.push_back(prior.comb);
    if (!topk) pl.add("pose.argmax", am_uses, [=](const Ctx& c) { issue_pose_argmax(wt.at(c), prior.call(c), B, c.stream); }, 0, 4.0 * B * 262144.0);
    if (pl.key.credible) {
        tt.cstate = pl.alloc(1, 1, 1, (int)credible_state_words(B));
        tt.ctoff = pl.alloc_tickets((size_t)B); tt.czoff = pl.alloc_tickets(credible_zero_words(B));
        const TailTensors wc = tt;
        pl.add("pose.credible", {tt.logits, tt.part, tt.cstate}, [=](const Ctx& c) { issue_pose_credible(wc.at(c), prior.call(c), nullptr, B, c.stream); },
               0, 4.0 * B * 262144.0 * (CRED_PASSES + 1));
    }
}

// Full plans: the softmax over the caller's logits into the caller's heatmap
static void add_softmax(Plan& pl, int B) {
    Tensor part = pl.alloc(B, 1, TAIL_CHUNKS, 2);
    pl.add("softmax", {part}, [=](const Ctx& c) {
        SoftmaxParams p{};
        p.logits = c.out.logits_flattened; p.B = B; p.n = CCVPE_OUT_HW * CCVPE_OUT_HW; p.partial = c.ptr(part); p.chunks = TAIL_CHUNKS;
        p.out = c.out.heatmap;
        launch_softmax(p, c.stream);
    }, 0, 4.0 * B * 262144.0 * 3);
}

// Heading-prior plans: pose.hprior (kernels_hprior.hip) writes the combined map `comb` from the orientation field `of`, the call's
// heading table and its position prior.  The name prefix keeps it on stream 0 (Plan::schedule), where it waits for the field's launch
// of stream 1 - a dependency from the tensor lists.
static void add_hprior_map(Plan& pl, int B, Tensor of, Tensor comb) {
    pl.add("pose.hprior", {of, comb}, [=](const Ctx& c) {
        HeadingPriorMapParams p{};
        p.ori = c.ptr(of); p.prior = c.tail.log_prior; p.prior_stride = c.tail.prior_stride; p.table = c.tail.hprior_table;
        p.table_stride = c.tail.hprior_stride; p.nb = c.tail.hprior_nb; p.out = c.ptr(comb); p.B = B;
        launch_heading_prior_map(p, c.stream);
    }, 0, 4.0 * B * 262144.0 * 4);
}

// rows[2..4] from the whole orientation field in the workspace, at the argmax (ori1.gather) or at the K peaks (ori1.topk_gather)
static void add_ori_gather(Plan& pl, int B, Tensor of, Tensor idx, bool topk) {
    if (topk) pl.add("ori1.topk_gather", {of, idx}, [=](const Ctx& c) {
        launch_topk_gather(c.ptr(of), reinterpret_cast<const int*>(c.ptr(idx)), B, c.tail.topk_k, CCVPE_OUT_HW * CCVPE_OUT_HW, c.tail.rows, c.stream);
    }, 0, 12.0 * B * 8);
    else pl.add("ori1.gather", {of, idx}, [=](const Ctx& c) {
        launch_pose_gather(c.ptr(of), reinterpret_cast<const int*>(c.ptr(idx)), B, CCVPE_OUT_HW * CCVPE_OUT_HW, c.tail.rows, c.stream);
    }, 0, 12.0 * B);
}

// pose.heading (kernels_heading.hip): reads the logits, the softmax partials, the argmax and the field, so it waits for both
// streams' tails.  The float64 hand-off lives in the workspace; the queries' fixed-point histograms must be zero between
// launches like the counters, so they live beside them (never in the arena, which the autotuner fills).
static void add_pose_heading(Plan& pl, int B, Tensor ori_field, const TailPrior prior, TailTensors& tt) {
    static_assert(sizeof(double) == 2 * sizeof(float) && sizeof(unsigned long long) == 2 * sizeof(unsigned), "allocated in words");
    tt.ori = ori_field;
    tt.hpart = pl.alloc(B, 1, TAIL_CHUNKS, 2 * HEADING_PART);
    tt.htoff = pl.alloc_tickets((size_t)B); tt.boff = pl.alloc_tickets((size_t)B * HEADING_MAX_BINS * 2);
    std::vector<Tensor> hd_uses = {tt.logits, tt.part, tt.index, tt.ori, tt.hpart};
    if (prior.comb.id >= 0) hd_uses.push_back(prior.comb);
    const TailTensors w = tt;
    pl.add("pose.heading", hd_uses, [=](const Ctx& c) { issue_pose_heading(w.at(c), prior.call(c), B, c.stream); }, 0, 4.0 * B * 262144.0 * 3);
}

// Aerial-encode plans: an encoder tap into its section of the caller's cache
static void add_tap_to_cache(Plan& pl, const std::string& name, Tensor tp, size_t o, size_t n) {
    pl.add(name, {tp}, [=](const Ctx& c) {
        (void)hipMemcpyAsync(c.cache_out + o, c.ptr(tp), n * sizeof(float), hipMemcpyDeviceToDevice, c.stream);
    }, 0, 8.0 * n);
}

// ------------------------------------------------------------------------------------------------
// The plan builder: what the stages of a plan hand to each other, and the stages in the order build_plan runs them.
// A stage decides and allocates; it holds no lambda - every launch comes from a description above - so no closure can capture the
// builder, which is gone when the plan first runs.
// ------------------------------------------------------------------------------------------------
struct PlanBuilder {
    ccvpe_handle_s* const h;
    Plan& pl;
    const VariantSpec& vs;
    const int B, gh, gw;
    // the normalised key: pose plans (ccvpe_localize*) hold the launches of the full (mode 0) or cached (mode 2) plan up to and including
    // the level-2 decoders, under the same names - so the same tuning-table entries - and a tail that writes result rows only
    const bool pose, topk, heading, hprior;
    const bool cached, grd_cached;   // the aerial side from an aerial cache (modes 2, 4); pair plans: the ground side from a ground cache too
    const bool circular;
    int fh = 0, fw = 0, L[6] = {0}, ltot = 0, loff[6] = {0};   // the ground feature volume and the levels' descriptor lengths and offsets
    Tensor loc_in[6], ori_in6;          // deconv inputs: [score pad 8 | C]; the orientation decoder's [rfull scores | pad to rpad | D]
    Tensor loc_cat[6], ori_cat[6];      // deconv out + skip (level index j = 0..5 <-> decoder level 6-j)
    Level6Form l6;
    EncOut genc, senc;
    Tensor desc, dmap;                  // the ground descriptors [B][ltot], the aerial descriptor map [B, 8, 8, D]
    MatchPrep prep;
    Tensor loc_mid, logits_ws;          // unfused level 1: conv_a's output; pose plans: the logits stay in the workspace
    Tensor comb;                        // heading-prior plans: the combined prior map
    TailTensors tt;
    Tensor raw, ori_x, ori_field;       // debug full plans: ori_level1_nchw; the orientation level 1's input; pose plans: the field in the workspace

    PlanBuilder(ccvpe_handle_s* h_, Plan& pl_)
        : h(h_), pl(pl_), vs(h_->vs), B(pl_.key.B), gh(pl_.key.gh), gw(pl_.key.gw), pose(pl_.key.pose), topk(pl_.key.topk), heading(pl_.key.heading),
          hprior(pl_.key.hprior), cached(pl_.key.mode == 2 || pl_.key.mode == 4), grd_cached(pl_.key.mode == 4), circular(h_->cfg.circular_padding != 0) {}

    // The split-K scratch and - full plans - the second stream's, the schedule's switches and the staging buffers of a replayed plan.
    // hipGraph replay: opt-in since round 4 (CCVPE_GRAPH=1).  Rounds 2-3 replayed plans of <= 4 samples: with ~330 launches per frame the
    // host could not keep up.  A batch-1 frame is 137 launches now; issued eagerly (interleaved over the two streams, Plan::schedule) the
    // GPU starts on the first while the host still hands over the rest, and a synchronised frame takes 1.31 ms against 1.44 ms replayed
    // (the replay's set-up precedes its first kernel); back to back both run at the GPU's pace.  Cached and pose plans are never
    // captured into a hipGraph.
    void staging(bool full) {
        pl.debug = full && h->debug;
        pl.no_reuse = h->sw.no_reuse;
        pl.scratch = pl.alloc(1, 1, 1, (int)Plan::SPLITK_FLOATS);
        if (!full) return;
        pl.two_streams = h->sw.two_streams && !h->debug;
        pl.issue_interleaved = h->sw.issue_interleaved; pl.log_schedule = h->sw.log_schedule;
        if (pl.two_streams) pl.scratch2 = pl.alloc(1, 1, 1, (int)Plan::SPLITK_FLOATS);
        pl.use_graph = !cached && !pose && h->sw.graph_mode == 1;
        if (!pl.use_graph) return;
        pl.io_grd = pl.alloc(B, 3, gh, gw);
        pl.io_sat = pl.alloc(B, 3, CCVPE_SAT_HW, CCVPE_SAT_HW);
        pl.io_logits = pl.alloc(B, 1, CCVPE_OUT_HW, CCVPE_OUT_HW);
        pl.io_heat = pl.alloc(B, 1, CCVPE_OUT_HW, CCVPE_OUT_HW);
        pl.io_ori = pl.alloc(B, 2, CCVPE_OUT_HW, CCVPE_OUT_HW);
        for (int k = 0; k < 6; ++k) pl.io_ms[k] = pl.alloc(B, h->rolls[k], 8 << k, 8 << k);
    }

    int geometry() {
        if (int rc = grd_geometry(vs, circular, gh, gw, fh, fw, L)) return rc;
        for (int k = 0; k < 6; ++k) { loff[k] = ltot; ltot += round_up(L[k], 4); }
        return 0;
    }

    // The decoder concat buffers: allocated first, the aerial encoder's tap epilogues write into them
    void concat_buffers() {
        for (int j = 0; j < 6; ++j) {
            const int hw_in = 8 << j;
            loc_in[j] = pl.alloc(B, hw_in, hw_in, 8 + vs.match_ch[j]);
            loc_cat[j] = pl.alloc(B, hw_in * 2, hw_in * 2, deconv_width(vs.loc[j], h->sw.pad_concat) + vs.loc[j].skip);
            ori_cat[j] = pl.alloc(B, hw_in * 2, hw_in * 2, deconv_width(vs.ori[j], h->sw.pad_concat) + vs.ori[j].skip);
            // bf16x3 mode: tensors consumed only by convolutions live as pre-split bf16 planes (same bytes), so the
            // consumers' K loops carry no fp32->bf16 conversion; level 1 (j == 5) feeds the fp32 tail and stays fp32
            if (h->cfg.reserved[0] == 1 && j < 5 && h->sw.split_planes) { loc_cat[j].split = true; ori_cat[j].split = true; }
        }
    }

    // Level 6 composed (kernels_level6.hip): fp32 plans on a handle with weights; automatic from LEVEL6_AUTO_MIN_BATCH
    // samples (batch-1 plans keep the three launches and their launch count), CCVPE_COMPOSE_L6 = 0 / 1 / 2 never / always / always as
    // F(2x2,2x2).  The level-6 concat buffers are then never written: block 15 keeps its own dense tensor only.  Only the shapes are
    // needed here (level6_shape: no device work, so a size query stays one); get_plan derives the weights before the plan first runs,
    // and where that fails under the automatic rule it builds the plan again with the three launches (h->l6_failed).
    // Then the orientation decoder's level-6 input, behind the decision as it always was.
    int level6_form() {
        const int rpad = score_pad(vs.n_rolls), D = vs.sat_desc;
        const bool forced = h->sw.compose_l6 && (*h->sw.compose_l6 == 1 || *h->sw.compose_l6 == 2);
        l6.wm = !h->finalized || h->cfg.reserved[0] != 0 || !h->sw.wino ? 0
                : h->sw.compose_l6 ? (*h->sw.compose_l6 == 1 ? 4 : *h->sw.compose_l6 == 2 ? 2 : 0)
                : (B >= LEVEL6_AUTO_MIN_BATCH && !h->l6_failed) ? 4 : 0;
        if (l6.wm) {
            bool ok = true;
            for (int d = 0; d < 2; ++d) {
                Level6Params& q = l6.p[d];
                q.wm = l6.wm; q.B = B; q.groups = 4 * level6_positions(l6.wm);
                ok = ok && level6_shape(h, d ? h->ori : h->loc, d ? vs.ori[0] : vs.loc[0], q.K, q.Kc, q.N, q.Npad) == 0;
                q.R = level6_rows(B, l6.wm, &q.bm);
                ok = ok && level6_supported(q) && q.K == (d ? rpad + D : loc_in[0].C);
            }
            if (!ok && forced) return ccvpe_fail(CCVPE_ESTATE, "composed level 6: the packed weights do not fit the plan's level-6 inputs");
            if (!ok) l6.wm = 0;
        }
        // conv6.2 and the skip half in split form (CCVPE_SPLIT_L6): only beside the composed level 6 - the skip half is a layer of its
        // own only there; a layer whose sizes the kernels do not take keeps its tiled launch
        if (l6.wm) {
            const int both = SPLIT6_CONV_B | SPLIT6_SKIP, sw = h->sw.split_l6 ? *h->sw.split_l6 : -1;
            const int want = sw >= 0 ? (sw == 1 ? both : sw == 2 ? SPLIT6_CONV_B : sw == 3 ? SPLIT6_SKIP : 0)
                             : (B >= LEVEL6_SPLIT_MIN_BATCH && !h->l6_split_failed) ? both : 0;
            for (int bit : {SPLIT6_CONV_B, SPLIT6_SKIP}) {
                if (!(want & bit)) continue;
                bool ok = true;
                for (int d = 0; d < 2; ++d) {
                    const DecLevel& l = d ? vs.ori[0] : vs.loc[0];
                    Split6Params& q = bit == SPLIT6_CONV_B ? l6.sb[d] : l6.ss[d];
                    q = Split6Params{};
                    q.B = B; q.C = bit == SPLIT6_CONV_B ? l.mid : l.skip; q.Kc = round_up(q.C, 32);
                    q.N = bit == SPLIT6_CONV_B ? l.out : l.mid; q.Npad = round_up(q.N, 128);
                    q.R = split6_rows(B, &q.bm);
                    q.x_ld = q.C; q.x_coff = 0; q.out_ld = q.N; q.out_coff = 0;   // dense tensors on both sides
                    const PackedConv& pc = bit == SPLIT6_CONV_B ? (d ? h->ori : h->loc).convb[0] : (d ? h->ori : h->loc).conva[0];
                    ok = ok && split6_supported(q) && pc.w != nullptr && (bit == SPLIT6_CONV_B ? pc.N == q.N && pc.cinp == q.C : l6.p[d].N == q.N);
                }
                if (ok) l6.split |= bit;
            }
        }
        pl.l6_wm = l6.wm;
        pl.l6_split = l6.split;
        ori_in6 = pl.alloc(B, 8, 8, rpad + D);
        pl.taps["ori_in6"] = {ori_in6, 0, ori_in6.C};   // (read by debug handles only, like every tap: [rfull scores | pad to rpad | D])
        return 0;
    }

    // The ground encoder: the same launches, names and shapes in the full, the cached and the ground-encode plan (the encoder's
    // latency-plan spread depends on the ground geometry only).  Pair plans have none.
    void ground_encoder() { plan_encoder(h, pl, h->grd_enc, true, B, gh, gw, circular, nullptr, genc, "grd"); }

    // The aerial encoder, its tap epilogues writing the skip halves of the decoder concat buffers - or, cached plans, the five launches
    // that read those sections of the aerial cache (block 15 of a composed level 6: one dense copy instead of the two concat slices)
    void aerial_side() {
        TapDst td[5];
        for (int t = 0; t < 5; ++t) {
            td[t].n = 2;
            td[t].t[0] = loc_cat[t]; td[t].coff[0] = deconv_width(vs.loc[t], h->sw.pad_concat);
            td[t].t[1] = ori_cat[t]; td[t].coff[1] = deconv_width(vs.ori[t], h->sw.pad_concat);
        }
        if (l6.wm) td[0].n = 0;
        if (!cached) {
            plan_encoder(h, pl, h->sat_enc, false, B, CCVPE_SAT_HW, CCVPE_SAT_HW, false, td, senc, "sat");
            l6.skip15 = senc.tap[TAP_BLOCK[0]];
            return;
        }
        if (l6.wm) l6.skip15 = pl.alloc(B, 16, 16, TAP_C[0]);
        size_t coff[6], one[6];
        cache_layout(vs, B, coff);
        cache_layout(vs, 1, one);
        for (int t = 0; t < 5; ++t) {
            const std::string name = "sat.cached_tap" + std::to_string(TAP_BLOCK[t]);
            const int C = TAP_C[t];
            const long long P = (long long)B * TAP_HW[t];
            if (t == 0 && l6.wm) add_cache_read(pl, name, B, coff[1], one[1], C, TAP_HW[t], l6.skip15, 0, Tensor{}, 0, 4.0 * P * C * 2);
            else add_cache_read(pl, name, B, coff[t + 1], one[t + 1], C, TAP_HW[t], td[t].t[0], td[t].coff[0], td[t].t[1], td[t].coff[1], 4.0 * P * C * 3);
        }
    }

    // grd.heads + grd.desc over the ground encoder's volume - to_cache: into the caller's ground cache (ccvpe_encode_ground).
    // Pair plans (mode 4, ccvpe_localize_region): the cached pose plan with the ground side from a ground cache as well - the ground
    // encoder, grd.heads and grd.desc give way to grd.cached_desc, a gather of each pair's query row (Ctx::query_index); the aerial
    // launches gather each pair's tile (Ctx::tile_index).  Every other launch keeps the cached pose plan's name and tuning entry.
    void ground_descriptors(bool to_cache) {
        if (grd_cached) { desc = pl.alloc(B, 1, 1, ltot); add_ground_cache_read(pl, B, ltot, desc); }
        else desc = plan_grd_desc(h, pl, B, fh, fw, genc.vol, to_cache);
        if (!to_cache) for (int k = 0; k < 6; ++k) pl.taps["grd_desc" + std::to_string(k + 1)] = {desc, loff[k], L[k]};
    }

    // The aerial descriptor map, from the encoder's volume or from the cache's first section (offset 0 whatever n_tiles is)
    void descriptor_map() {
        const int D = vs.sat_desc;
        dmap = pl.alloc(B, 8, 8, D);
        const long long P = (long long)B * 64;
        if (cached) add_cache_read(pl, "sat.cached_descmap", B, 0, 0, D, 64, dmap, 0, Tensor{}, 0, 8.0 * P * D);
        else add_descmap(h, pl, B, senc.vol, dmap);
        pl.taps["sat_descriptor_map"] = {dmap, 0, D};
    }

    // The six matching levels, each followed by the localisation decoder's level it feeds; the last decoder level is the fused launch
    // (pose plans: into the workspace) or, unfused, ends at conv_a's output (loc_mid).  Pose plans write no matching-score stacks.
    void matching_levels() {
        Tensor x = dmap;
        logits_ws = pose ? pl.alloc(B, 1, CCVPE_OUT_HW, CCVPE_OUT_HW) : Tensor{};
        for (int k = 0; k < 6; ++k) {
            MatchParams mp = match_level_params(vs, h->cfg, k, L[k]);
            mp.x_ld = x.C; mp.B = B; mp.g_ld = ltot;
            mp.no_wide = h->sw.match_wide ? 0 : 1;
            mp.prep_done = h->sw.match_prep_early ? 1 : 0;
            if (k == 0) prep.first_op = pl.ops.size();
            add_match(pl, k, mp, pose, x, desc, loff[k], loc_in[k], k == 0 ? ori_in6 : Tensor{}, h->sw.match_prep_early ? &prep : nullptr);
            pl.taps["loc_in" + std::to_string(6 - k)] = {loc_in[k], 0, loc_in[k].C};
            if (k == 5 && h->sw.fuse_level1) { plan_level1_fused(h, pl, B, h->loc, loc_in[k], vs.loc[5].din, 1, false, Tensor{}, "loc1", logits_ws); break; }
            Tensor o = plan_level(h, pl, B, l6, h->loc, vs.loc, k, loc_in[k], loc_cat[k], "loc" + std::to_string(6 - k));
            if (k < 5) { pl.taps["loc_level" + std::to_string(6 - k)] = {o, 0, o.C}; x = o; }
            else loc_mid = o;
        }
    }

    // Behind the logits.  Pose plans: the tail (add_pose_tail) - but a heading-prior plan (ccvpe_localize_heading_prior*, DESIGN.md 4.16:
    // the heading plan plus the workspace map `comb`) only allocates the map here: its tail reads `comb`, which pose.hprior writes
    // from the orientation field, so its launches are added behind the orientation decoder's whole-field launch (orientation_level1);
    // every other plan adds them here, in the program order it always had.  Full plans: the softmax.
    void pose_tail_or_softmax() {
        if (hprior) comb = pl.alloc(B, 1, CCVPE_OUT_HW, CCVPE_OUT_HW);
        if (pose && !hprior) add_pose_tail(pl, B, logits_ws, TailPrior{comb}, tt);
        if (!pose) add_softmax(pl, B);
    }

    // Orientation decoder levels 6 .. 2
    void orientation_levels() {
        if (h->debug && !pose) { raw = pl.alloc(B, 2, CCVPE_OUT_HW, CCVPE_OUT_HW); pl.taps["ori_level1_nchw"] = {raw, 0, -1}; }   // (pose plans have no debug taps: ccvpe_localize refuses a debug handle)
        ori_x = ori_in6;
        for (int j = 0; j < 5; ++j) {
            Tensor o = plan_level(h, pl, B, l6, h->ori, vs.ori, j, ori_x, ori_cat[j], "ori" + std::to_string(6 - j));
            pl.taps["ori_level" + std::to_string(6 - j)] = {o, 0, o.C};
            ori_x = o;
        }
    }

    // Orientation level 1, four forms:
    //  - pose and top-K plans with the fused level: the fused tile at the argmax / at each of the K peaks (ori1.pose / ori1.topk), no field;
    //  - heading plans (ccvpe_localize_heading*) with the fused level: the argmax pose plan with the WHOLE field in the
    //    workspace - the full plan's launch ori1.fused, the same name and shape, so the same tuning entry;
    //  - full plans with the fused level: the same launch to the caller;
    //  - without the fused level: ori1.deconv, ori1.conv_a and ori1.tail, to the caller or - pose plans - into the workspace.
    // A heading-prior plan then adds pose.hprior and its tail, behind the launch that writes the whole field; a pose plan that holds
    // the field reads rows[2..4] from it (ori1.gather, ori1.topk_gather).
    void orientation_level1() {
        if (h->sw.fuse_level1 && pose && !heading) { add_level1_peaks(h, pl, B, ori_x, tt.index, topk, vs.ori[5].din); return; }
        if (h->sw.fuse_level1) {
            if (pose) ori_field = pl.alloc(B, 2, CCVPE_OUT_HW, CCVPE_OUT_HW);
            plan_level1_fused(h, pl, B, h->ori, ori_x, vs.ori[5].din, 2, true, raw, "ori1", ori_field);
        } else {
            Tensor m = plan_level(h, pl, B, l6, h->ori, vs.ori, 5, ori_x, ori_cat[5], "ori1");
            if (pose) ori_field = pl.alloc(B, 2, CCVPE_OUT_HW, CCVPE_OUT_HW);
            add_tail_conv(pl, "ori1.tail", B, h->ori, 2, m, raw, ori_field);
        }
        if (hprior) { add_hprior_map(pl, B, ori_field, comb); add_pose_tail(pl, B, logits_ws, TailPrior{comb}, tt); }
        if (pose) add_ori_gather(pl, B, ori_field, tt.index, topk);
    }

    // The 2 GiB bound (the ground / aerial inputs and the 2 x 512 x 512 orientation output are addressed the same way), the two-stream
    // schedule, the workspace layout
    int finish() {
        if (tensor_too_large(pl, (size_t)B * 3 * std::max(gh * gw, CCVPE_SAT_HW * CCVPE_SAT_HW) * sizeof(float)))
            return ccvpe_fail(CCVPE_EINVAL, "micro-batch %d needs a %d x %d x %d x %d tensor of %zu bytes; the kernels address tensors with 32-bit byte offsets (< 2 GiB): "
                        "use a smaller micro_batch (ccvpe_max_micro_batch)", B, pl.max_dims[0], pl.max_dims[1], pl.max_dims[2], pl.max_dims[3], pl.max_tensor_bytes);
        pl.schedule();
        pl.assign();
        return 0;
    }
};

// Key normalisation (top-K and summary are forms of pose plans; a top-K plan has no summary) and the form refusals, before any allocation
static int normalise_key(Plan& pl, const PlanKey& key) {
    pl.key = key;
    pl.key.topk = key.pose && key.topk;
    pl.key.summary = key.pose && !key.topk && key.summary;
    if (key.credible && (!key.pose || key.topk || key.summary || key.heading || key.mode == 4))
        return ccvpe_fail(CCVPE_EINVAL, "credible plans are plain argmax pose plans (no top-K, no summary, no heading, no pairs)");
    if (key.heading && (!key.pose || key.topk || key.mode == 4)) return ccvpe_fail(CCVPE_EINVAL, "heading plans are argmax pose plans (no top-K, no pairs)");
    if (key.hprior && !key.heading) return ccvpe_fail(CCVPE_EINVAL, "heading-prior plans are heading plans");
    if (key.mode == 4 && (!key.pose || key.topk)) return ccvpe_fail(CCVPE_EINVAL, "pair plans are single-hypothesis pose plans");
    return 0;
}

// Ground-only plan (mode 3, ccvpe_encode_ground): the full plan's ground encoder, grd.heads and grd.desc, with grd.desc writing into
// the caller's ground cache
static int build_ground_plan(PlanBuilder& b) {
    if (int rc = b.geometry()) return rc;
    b.staging(false);
    b.ground_encoder();
    b.ground_descriptors(true);
    if (tensor_too_large(b.pl, (size_t)b.B * 3 * b.gh * b.gw * sizeof(float)))
        return ccvpe_fail(CCVPE_EINVAL, "ground encode of %d images needs a tensor of %zu bytes (< 2 GiB): use a smaller batch", b.B, b.pl.max_tensor_bytes);
    b.pl.assign();
    return 0;
}

// Aerial-only plan (mode 1, ccvpe_encode_aerial): the full plan's aerial encoder without tap destinations, sat.descmap and the five
// taps into the caller's cache (cache_layout)
static int build_aerial_plan(PlanBuilder& b) {
    Plan& pl = b.pl;
    b.staging(false);
    plan_encoder(b.h, pl, b.h->sat_enc, false, b.B, CCVPE_SAT_HW, CCVPE_SAT_HW, false, nullptr, b.senc, "sat");
    size_t coff[6];
    cache_layout(b.vs, b.B, coff);
    pl.tune_cache = pl.alloc(b.B, 8, 8, b.vs.sat_desc);
    add_descmap(b.h, pl, b.B, b.senc.vol, Tensor{});
    for (int t = 0; t < 5; ++t)
        add_tap_to_cache(pl, "sat.tap_to_cache" + std::to_string(TAP_BLOCK[t]), b.senc.tap[TAP_BLOCK[t]], coff[t + 1], (size_t)b.B * TAP_HW[t] * TAP_C[t]);
    pl.assign();
    return 0;
}

// A PlanKey into the list of launches: the refusals, the builder, the stages in order.  The order is behaviour.
int build_plan(ccvpe_handle_s* h, Plan& pl, const PlanKey& key) {
    if (int rc = normalise_key(pl, key)) return rc;
    PlanBuilder b(h, pl);
    if (key.mode == 1) return build_aerial_plan(b);
    if (key.mode == 3) return build_ground_plan(b);
    b.staging(true);
    if (int rc = b.geometry()) return rc;
    b.concat_buffers();
    if (int rc = b.level6_form()) return rc;
    if (!b.grd_cached) b.ground_encoder();
    b.aerial_side();
    b.ground_descriptors(false);
    b.descriptor_map();
    b.matching_levels();
    if (!b.prep.fills.empty()) add_match_prep(pl, b.prep);
    if (!h->sw.fuse_level1) add_tail_conv(pl, "loc1.tail", b.B, h->loc, 1, b.loc_mid, Tensor{}, b.logits_ws);
    b.pose_tail_or_softmax();
    b.orientation_levels();
    b.orientation_level1();
    if (b.heading) add_pose_heading(pl, b.B, b.ori_field, TailPrior{b.comb}, b.tt);
    return b.finish();
}
