// Body of level1_kernel and level1_pose_kernel (kernels_level1.hip), included inside both kernels.  In scope: `p` (Level1Params), COUT,
// NG and SCORE (the composed weights' shape; NG == 0: p.ng and p.score at run time), TILE (the output tile's shape and the workgroup's
// size, L1Shape), constexpr bool POSE, `pose_index` and `pose_rows` (null unless POSE),
// and the POSE addressing: the workgroup runs the tile of pixel pose_index[pose_slot] of sample pose_sample and writes row
// pose_rows[b * pose_ld + pose_r0 + 0..4].
// Everything below is a function of the tile shape; what is computed for one conv_a position or one output pixel is not (the K order of
// the composed GEMM, the bias / ReLU / zeroing, the order of the nine tail adds), so every shape gives every output the same bits.
constexpr int TY = L1Shape<TILE>::TY, TX = L1Shape<TILE>::TX, NTHR = L1Shape<TILE>::NTHR;   // output tile TY rows x TX columns
constexpr int ATY = TY + 2, ATX = TX + 2;             // conv_a-output tile (halo 1)
constexpr int XTY = TY / 2 + 2, XTX = TX / 2 + 2;     // input tile
constexpr int PS = l1_ps(COUT, TX);                   // floats per pixel in the P tile
constexpr int NPX = ATX / 2, NPOS = (ATY / 2) * NPX;  // conv_a pixels of one parity class: 9 x 9, or 9 rows of 17
constexpr int NPART = NTHR / 256;                     // waves per parity class: each takes NMT1 of the class's m-tiles
constexpr int NMT1 = ((NPOS + 15) / 16 + NPART - 1) / NPART;   // 6; 32 x 16: 10, or 5 in each of two waves
constexpr int XI_MAX = (XTY * XTX * KCH_MAX * 4 + NTHR - 1) / NTHR;   // float4 items per thread of one X tile
extern __shared__ __attribute__((aligned(16))) float smem[];
const int CXP = p.cxp;                 // input channels padded to a multiple of 16
const int XS = CXP + 4;                // row stride of the X tile
float* Xs = smem;                      // [XTY*XTX][XS]
float* Ps = smem + XTY * XTX * XS;    // [ATY*ATX][PS] the tail conv's per-tap products (its own region: two barriers per tile)

const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
const int H = p.H, W = p.W;            // output size (512); input is H/2 x W/2
const int IH = H >> 1, IW = W >> 1;
const int tiles_x = W / TX, tiles_y = H / TY;
const int tiles = p.B * tiles_x * tiles_y;
const int xcd = blockIdx.x & 7;
const int stride = ((int)gridDim.x >> 3) + (xcd < ((int)gridDim.x & 7) ? 1 : 0);
const int t_begin = xcd * (tiles >> 3) + min(xcd, tiles & 7);
int t_end = t_begin + (tiles >> 3) + (xcd < (tiles & 7) ? 1 : 0);
int tile = t_begin + ((int)blockIdx.x >> 3);
int pose_pix = 0;                      // POSE: the pixel (row * W + col) whose orientation this workgroup writes
if constexpr (POSE) {
    pose_pix = min(max(pose_index[pose_slot], 0), H * W - 1);
    tile = pose_sample * (tiles_x * tiles_y) + (pose_pix / W / TY) * tiles_x + (pose_pix % W) / TX;
    t_end = tile + 1;                  // one tile: no next one to prefetch
}
if (tile >= t_end) return;

// ---- once per workgroup ----
// Last conv (16 -> COUT, 3x3) in two steps (round 3): P[pixel][tap, co] = sum_c A[pixel][c] wt[tap][co][c] for every pixel of the 18 x 18
// conv_a tile - a [324 x 16] x [16 x 9 COUT] GEMM whose B operand is the conv_a accumulator AS IT STANDS in registers (lane = pixel,
// 4 channels: exactly the operand layout), 4 MFMAs per 16 pixels and 16 (tap, co) columns - and out[y][x][co] = bt + sum_tap P[(y + dy,
// x + dx)][tap, co]: nine LDS reads and adds per output.
constexpr int NPT = (9 * COUT + 15) / 16;                     // 16-column tiles of P
f32x4 wtf[NPT];                                               // A fragments: wt[n = 16 nt + (lane & 15)][4 (lane >> 4) + e], n = tap * COUT + co
#pragma unroll
for (int nt = 0; nt < NPT; ++nt) {
    const int n = nt * 16 + (lane & 15);
    wtf[nt] = n < 9 * COUT ? *reinterpret_cast<const f32x4*>(p.wt + (size_t)n * 16 + 4 * (lane >> 4)) : f32x4{0.f, 0.f, 0.f, 0.f};
}
// Composed transposed conv + conv_a (DESIGN.md 4.3): wave w computes conv_a pixels of parity class w & 3, (py, px) = (class >> 1, class & 1)
// - with 512 threads wave w takes m-tiles (w >> 2) * NMT1 .. of its class; position (i, j) of that class (9 x 9 per 16 x 16 tile, i =
// pos / NPX) is conv_a pixel (2i + 1 - py, 2j + 1 - px) of the conv_a tile and reads the 2 x 2 window of X
// tile pixels (i + a, j + b).  K order: the score k-step (if any), then descriptor group g = 0 .. ng-1, channel 4g + e, e = 0..3; in every
// k-step the lanes of quarter q = lane >> 4 read window (a, b) = (q >> 1, q & 1).  The weights are the A operand: lane = output channel
// lane & 15 of window q; the accumulator of a lane holds channels 4 (lane >> 4) .. + 3 of ONE position.
constexpr bool NG_RT = NG == 0;        // generic form: up to 16 groups, guarded (the width classes of the real variants are exact)
constexpr int NGR = NG_RT ? 16 : NG;   // register slots for the descriptor groups
const int ng = NG_RT ? p.ng : NG;
const bool score = NG_RT ? p.score != 0 : SCORE != 0;
const int cls = wave & 3, part = wave >> 2;
const float wsc = score ? p.ws[cls * 64 + lane] : 0.f;
f32x4 wg[NGR];
#pragma unroll
for (int g = 0; g < NGR; ++g)
    wg[g] = g < ng ? *reinterpret_cast<const f32x4*>(p.wc + ((size_t)(cls * ng + g) * 64 + lane) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
const f32x4 bint = *reinterpret_cast<const f32x4*>(p.bc + 4 * (lane >> 4));   // interior bias (table row 0)
const int py = cls >> 1, px = cls & 1;
int xoff[NMT1], pq[NMT1];   // per m-tile: this lane's X read offset (window q) and the P tile pixel of its accumulator column
#pragma unroll
for (int mt = 0; mt < NMT1; ++mt) {
    const int row = (part * NMT1 + mt) * 16 + (lane & 15);
    const int pos = min(row, NPOS - 1);                       // padding lanes of the last m-tile read a real position
    const int i = pos / NPX, j = pos % NPX;
    xoff[mt] = ((i + ((lane >> 4) >> 1)) * XTX + j + ((lane >> 4) & 1)) * XS + p.c0;
    pq[mt] = row < NPOS ? (2 * i + 1 - py) * ATX + 2 * j + 1 - px : -1;   // -1: padding lane, nothing stored
}

// X tile staging: float4 item i = tid + it*NTHR -> pixel i / c4n, channels 4*(i % c4n)
const int c4n = CXP >> 2;
const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, (unsigned)((size_t)p.B * IH * IW * p.x_ld * 4), 0x00020000);
int x_lds[XI_MAX], x_rc[XI_MAX];   // LDS float offset (-1: no item), (row << 8 | col) inside the X tile, channel in bits 16+
#pragma unroll
for (int it = 0; it < XI_MAX; ++it) {
    const int i = tid + it * NTHR;
    const int px_ = i / c4n, c4 = i - px_ * c4n;
    const bool live = i < XTY * XTX * c4n;
    x_lds[it] = live ? px_ * XS + c4 * 4 : -1;
    x_rc[it] = ((px_ / XTX) << 8) | (px_ % XTX) | ((c4 * 4 < p.cx ? c4 * 4 : 0x7fff) << 16);
}
f32x4 xv[XI_MAX];
#define CCVPE_L1_LOAD_X(tl)                                                                              \
{                                                                                                    \
    const int b_ = (tl) / (tiles_x * tiles_y);                                                       \
    const int r_ = (tl) - b_ * (tiles_x * tiles_y);                                                  \
    const int ty_ = r_ / tiles_x, tx_ = r_ - ty_ * tiles_x;                                          \
    const int xr0_ = ty_ * (TY / 2) - 1, xc0_ = tx_ * (TX / 2) - 1;                                   \
    _Pragma("unroll") for (int it = 0; it < XI_MAX; ++it) {                                          \
        const int xr = xr0_ + ((x_rc[it] >> 8) & 0xff), xc = xc0_ + (x_rc[it] & 0xff), ch = x_rc[it] >> 16; \
        const bool ok = x_lds[it] >= 0 && (unsigned)xr < (unsigned)IH && (unsigned)xc < (unsigned)IW && ch != 0x7fff; \
        const unsigned off = ok ? (unsigned)((((b_ * IH + xr) * IW + xc) * p.x_ld + ch) * 4) : 0x80000000u; \
        xv[it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, off, 0, 0)); \
    }                                                                                                \
}
CCVPE_L1_LOAD_X(tile);

const size_t hw = (size_t)H * W;

#if CCVPE_L1_CLOCK
unsigned long long clk[7] = {0, 0, 0, 0, 0, 0, 0}, tprev = __builtin_amdgcn_s_memtime();
int ntiles = 0;
#endif
while (true) {
#if CCVPE_L1_CLOCK
    ++ntiles;
#endif
    const int b = tile / (tiles_x * tiles_y);
    const int rem = tile - b * (tiles_x * tiles_y);
    const int Y0 = (rem / tiles_x) * TY, X0 = (rem % tiles_x) * TX;
    const bool interior = Y0 >= 2 && Y0 + TY + 2 <= H && X0 >= 2 && X0 + TX + 2 <= W;

    // ---- stage 0: this tile's input pixels registers -> LDS; start fetching the next tile's ----
#pragma unroll
    for (int it = 0; it < XI_MAX; ++it)
        if (x_lds[it] >= 0) *reinterpret_cast<f32x4*>(Xs + x_lds[it]) = xv[it];
    __syncthreads();
    CCVPE_L1_STAMP(0);
    const int tile_n = tile + stride;
    const bool have_n = tile_n < t_end;
    if (have_n) { CCVPE_L1_LOAD_X(tile_n); }

    // ---- stage 1: conv_a of this wave's parity class as one GEMM [NPOS x K] x [K x 16], K = 4 (score + 4 ng): NMT1 independent chains ----
    f32x4 acc[NMT1];
#pragma unroll
    for (int mt = 0; mt < NMT1; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (score) {
#pragma unroll
        for (int mt = 0; mt < NMT1; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wsc, Xs[xoff[mt] - p.c0], acc[mt], 0, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < NGR; ++g) {
        if (!NG_RT || g < ng) {   // (a guard, not a break: the loop must unroll fully so that wg stays in registers)
            f32x4 a[NMT1];
#pragma unroll
            for (int mt = 0; mt < NMT1; ++mt) a[mt] = *reinterpret_cast<const f32x4*>(Xs + xoff[mt] + 4 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int mt = 0; mt < NMT1; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wg[g][e], a[mt][e], acc[mt], 0, 0, 0);
        }
    }
    CCVPE_L1_STAMP(1);

    // ---- stage 2: bias (by border case) + ReLU + zero outside the image, then the tail conv's per-tap products into the P tile ----
#pragma unroll
    for (int mt = 0; mt < NMT1; ++mt) {
        const int q = max(pq[mt], 0);                               // P pixel of this lane's accumulator column
        f32x4 v;
        if (interior) {
            v = acc[mt] + bint;
        } else {
            const int gy = Y0 - 1 + q / ATX, gx = X0 - 1 + q % ATX;
            const int bcase = (gy == 0 ? 3 : gy == H - 1 ? 6 : 0) + (gx == 0 ? 1 : gx == W - 1 ? 2 : 0);
            v = acc[mt] + *reinterpret_cast<const f32x4*>(p.bc + bcase * 16 + 4 * (lane >> 4));
            if (!((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W)) v = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
        // the last conv's per-tap dot products of this pixel: v is the B operand as it stands
#pragma unroll
        for (int nt = 0; nt < NPT; ++nt) {
            f32x4 pa = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) pa = __builtin_amdgcn_mfma_f32_16x16x4f32(wtf[nt][e], v[e], pa, 0, 0, 0);
            // columns 16 nt + 4 (lane >> 4) .. + 3 of pixel q; 9 COUT <= 18 columns are real: the second tile keeps two
            if (pq[mt] >= 0) {
                float* pd = Ps + q * PS + 4 * (lane >> 4);
                if (nt == 0) {
                    if constexpr (PS % 4 == 0) {
                        *reinterpret_cast<f32x4*>(pd) = pa;
                    } else if constexpr (PS % 2 == 0) {   // 8-byte aligned pixels
                        *reinterpret_cast<f32x2*>(pd) = f32x2{pa[0], pa[1]};
                        *reinterpret_cast<f32x2*>(pd + 2) = f32x2{pa[2], pa[3]};
                    } else {                              // COUT 1, odd stride: the nine real columns
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (4 * (lane >> 4) + e < 9 * COUT) pd[e] = pa[e];
                    }
                } else if ((lane >> 4) == 0) *reinterpret_cast<f32x2*>(Ps + q * PS + 16) = f32x2{pa[0], pa[1]};
            }
        }
    }
    CCVPE_L1_STAMP(2);
    __syncthreads();
    CCVPE_L1_STAMP(3);

    // ---- stage 3: out = bias + the nine taps' dot products of the shifted pixels, TY * TX / NTHR output pixels per thread, NCHW store ----
#pragma unroll
    for (int r = 0; r < TY * TX / NTHR; ++r) {
        const int oy = (tid + r * NTHR) / TX, ox = (tid + r * NTHR) % TX;
        float o[COUT];
#pragma unroll
        for (int c = 0; c < COUT; ++c) o[c] = p.bt[c];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float* pp = Ps + ((oy + t / 3) * ATX + ox + t % 3) * PS + t * COUT;
            if (COUT == 2) { const f32x2 v = *reinterpret_cast<const f32x2*>(pp); o[0] += v.x; o[COUT - 1] += v.y; }
            else o[0] += pp[0];
        }
        const size_t opix = (size_t)(Y0 + oy) * W + X0 + ox;
        if (p.raw) {
#pragma unroll
            for (int c = 0; c < COUT; ++c) p.raw[((size_t)b * COUT + c) * hw + opix] = o[c];
        }
        if (p.normalize) {
            float n2 = 0.f;
#pragma unroll
            for (int c = 0; c < COUT; ++c) n2 = fmaf(o[c], o[c], n2);
            const float inv = 1.f / fmaxf(sqrtf(n2), 1e-12f);
#pragma unroll
            for (int c = 0; c < COUT; ++c) o[c] *= inv;
        }
        if constexpr (POSE) {   // (p.raw is null and p.normalize 1: the values ccvpe_postprocess_rows reads from the orientation output)
            static_assert(COUT == 2, "the pose form serves the orientation decoder");
            if (opix == (size_t)pose_pix) {
                pose_rows[b * pose_ld + pose_r0 + 2] = o[0];
                pose_rows[b * pose_ld + pose_r0 + 3] = o[1];
                pose_rows[b * pose_ld + pose_r0 + 4] = pose_angle_deg(o[0], o[1]);
            }
        } else {
#pragma unroll
            for (int c = 0; c < COUT; ++c) p.out[((size_t)b * COUT + c) * hw + opix] = o[c];
        }
    }
    if constexpr (POSE) break;

    CCVPE_L1_STAMP(4);
    if (!have_n) break;
    // (no barrier: the next tile's X stores follow every wave's stage-1 reads of this tile across the barrier above, and its P stores
    // follow the stage-3 reads of this tile across the barrier behind stage 0)
    tile = tile_n;
}
#if CCVPE_L1_CLOCK
if (lane == 0) {
    for (int i = 0; i < 7; ++i) atomicAdd(&g_l1_clk[i], clk[i]);
    atomicAdd(&g_l1_clk[7], 1ull);
    atomicAdd(&g_l1_clk[8], (unsigned long long)ntiles);
}
#endif
#undef CCVPE_L1_LOAD_X
