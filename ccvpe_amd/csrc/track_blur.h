// The blur passes and the log store track_predict_kernel (kernels_track.hip) and track_predict_affine_kernel (kernels_track_affine.hip)
// share: one definition, so that the affine kernel at an integer translation gives track_predict_kernel's bits.  The
// smoother (kernels_track_smooth.hip) runs the same passes on its two maps, so its motion model is the filter's bit
// for bit; the affine smoother (kernels_track_smooth_affine.hip) runs them behind the affine kernel's sampling and on
// its ratio map.  The files that include this are built with -fno-slp-vectorize (ccvpe_amd/build.py).
#pragma once
#include "kernels.h"

namespace ccvpe {

static constexpr int TRACK_T = 32;                 // tile side
static constexpr int TRACK_TILES = (TAIL_HW / TRACK_T) * (TAIL_HW / TRACK_T);   // 256 per query: one per CU at batch 1

// ---- a tile's source under a shift: the LDS layout of track_predict_kernel and of the smoother's two blur phases ----
__host__ __device__ constexpr int track_side(int r) { return TRACK_T + 2 * r + 1; }
// row pitch of the staged source: S is odd; P = 1 (mod 4) keeps the x pass (8 lanes per row, 4 columns apart) free of bank conflicts
__host__ __device__ constexpr int track_pitch(int r) { return (track_side(r) & 3) == 1 ? track_side(r) : track_side(r) + 2; }
// merged weights of one pass, zero-padded by 3 on both sides for the x pass' four outputs per thread
__host__ __device__ constexpr int track_wlen(int r) { return 2 * r + 2 + 6; }
static size_t track_lds_bytes(int r) { return sizeof(float) * ((size_t)track_side(r) * TRACK_T + 2 * track_wlen(r) + (size_t)track_side(r) * track_pitch(r)); }

// ---- a tile's source without a merged shift: the LDS layout of track_predict_affine_kernel and of the affine smoother's blur phases ----
__host__ __device__ constexpr int affine_side(int r) { return TRACK_T + 2 * r; }
// row pitch of the samples: S is even; an odd pitch puts the x pass' 32 lanes (4 rows, 8 lanes per row, 4 columns apart) on 32 banks
__host__ __device__ constexpr int affine_pitch(int r) { return affine_side(r) + 1; }
// two-sided weights, zero-padded by 3 on both sides for the x pass' four outputs per thread
__host__ __device__ constexpr int affine_wlen(int r) { return 2 * r + 1 + 6; }
static size_t affine_lds_bytes(int r) { return sizeof(float) * ((size_t)affine_side(r) * TRACK_T + affine_wlen(r) + (size_t)affine_side(r) * affine_pitch(r)); }

// The LDS of a shifted tile, carved out of track_lds_bytes(r) bytes (16-byte aligned)
struct TrackTile {
    float* mid;   // [S][32] x-pass result (16-byte aligned rows)
    float* wx;    // [WL] merged weights along x, wx[3 + k] = u[k]
    float* wy;    // [WL] along y
    float* src;   // [S][P] staged source
    int S, P;
};
__device__ __forceinline__ TrackTile track_tile(unsigned char* smem, int r) {
    TrackTile t;
    t.S = track_side(r); t.P = track_pitch(r);
    t.mid = reinterpret_cast<float*>(smem);
    t.wx = t.mid + t.S * TRACK_T;
    t.wy = t.wx + track_wlen(r);
    t.src = t.wy + track_wlen(r);
    return t;
}
// Every thread of the workgroup: the merged weights of the shift sign * shift[b] and the S x S source pixels of maps[b] [512][512] that
// the tile at (X0, Y0) needs, zeros outside the grid; the caller meets at a barrier before the passes.  Every global read is bounds-
// checked against the grid, and the integer part of the shift is clamped before it is converted, so no input value moves a read outside
// the map.  This is the staging of track_predict_kernel, statement for statement (sign = 1: the same weights and the same pixels);
// that kernel keeps its own text of it, because behind this call the compiler orders six of its scalar instructions differently and
// its instruction stream is held to the one measured in DESIGN.md 4.11.
__device__ __forceinline__ void track_stage_shifted(const TrackTile& t, const float* maps, const float* shift, float sign, const float* tap_sets,
                                                    int taps_stride, int b, int r, int Y0, int X0) {
    constexpr int HW = TAIL_HW, n = HW * HW;
    const int tid = threadIdx.x;
    const int S = t.S, P = t.P, WL = track_wlen(r);
    const float dx = sign * shift[b * 2 + 0], dy = sign * shift[b * 2 + 1];
    const float fdx = floorf(dx), fdy = floorf(dy);
    // integer part clamped to +-2048 (beyond +-544 nothing of the grid is left in reach; NaN clamps to -2048): the conversion is defined
    const int ix = (int)fminf(fmaxf(fdx, -2048.f), 2048.f), iy = (int)fminf(fmaxf(fdy, -2048.f), 2048.f);
    const float fx = dx - fdx, fy = dy - fdy;         // exact for finite shifts, in [0, 1)
    const float* taps = tap_sets + (size_t)b * taps_stride;
    if (tid < 2 * WL) {
        const bool y = tid >= WL;
        const int k = (y ? tid - WL : tid) - 3;
        const float f = y ? fy : fx;
        float u = 0.f;
        if (k >= 0 && k <= 2 * r + 1) {
            const int a = k - r < 0 ? r - k : k - r, c = k - 1 - r < 0 ? r + 1 - k : k - 1 - r;   // |k - r|, |k - 1 - r|
            const float ta = a <= r ? taps[a] : 0.f, tc = c <= r ? taps[c] : 0.f;
            u = fmaf(f, ta, (1.f - f) * tc);
        }
        (y ? t.wy : t.wx)[k + 3] = u;
    }
    // source rows gy0 .. gy0 + S - 1, columns gx0 .. gx0 + S - 1: a wave per row, lanes along the row
    const float* bel = maps + (size_t)b * n;
    const int gx0 = X0 - ix - r - 1, gy0 = Y0 - iy - r - 1;
    const int lane = tid & 63, wave = tid >> 6;
    for (int ly = wave; ly < S; ly += 4) {
        const int gy = gy0 + ly;
        const bool rowin = (unsigned)gy < (unsigned)HW;
        for (int lx = lane; lx < S; lx += 64) {
            const int gx = gx0 + lx;
            t.src[ly * P + lx] = rowin && (unsigned)gx < (unsigned)HW ? bel[gy * HW + gx] : 0.f;
        }
    }
}

// A workgroup of 256 threads behind the barrier that completed its staged source src [S][P] (row pitch P) and the weights of a pass,
// wx[3 + k] and wy[3 + k], k = 0 .. 2r + MERGED, zero-padded by 3 on both sides for the x pass' four outputs per thread: the 2r + 1
// taps of the blur, or with MERGED = 1 the 2r + 2 of the blur merged with a 2-tap shift.  x pass out of src into mid [S][32] (16-byte
// aligned rows), y pass out of that: thread tid gets the blur at row tid >> 3, columns (tid & 7) * 4 .. + 3 of the tile as one float4.
// A pass is that many fused multiply-adds per output in ascending source index from a zero accumulator.
template <int MERGED, bool LOG_STORE>
__device__ __forceinline__ auto track_blur_tile(const float* src, int S, int P, float* mid, const float* wx, const float* wy, int r,
                                                const float* floor, float* log_prior, int b, int Y0, int X0) {
    constexpr int HW = TAIL_HW, n = HW * HW;
    const int tid = threadIdx.x;
    // x pass: task = (row, 4 adjacent columns); source column x4 + c feeds output i with weight wx[3 + c - i]
    for (int i = tid; i < S * (TRACK_T / 4); i += 256) {
        const int ly = i >> 3, x4 = (i & 7) * 4;
        const float* row = src + ly * P + x4;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        float w1 = 0.f, w2 = 0.f, w3 = 0.f;          // the weights of outputs 1 .. 3 for this column: wx[3 + c - 1], [.. - 2], [.. - 3]
        for (int c = 0; c <= 2 * r + MERGED + 3; ++c) {
            const float v = row[c], w0 = wx[3 + c];
            a0 = fmaf(w0, v, a0); a1 = fmaf(w1, v, a1); a2 = fmaf(w2, v, a2); a3 = fmaf(w3, v, a3);
            w3 = w2; w2 = w1; w1 = w0;
        }
        *reinterpret_cast<float4*>(mid + ly * TRACK_T + x4) = make_float4(a0, a1, a2, a3);
    }
    __syncthreads();
    // y pass: thread = (output row, 4 adjacent columns)
    const int y = tid >> 3, x4 = (tid & 7) * 4;
    const float4* col = reinterpret_cast<const float4*>(mid + y * TRACK_T + x4);
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k <= 2 * r + MERGED; ++k) {
        const float4 v = col[k * (TRACK_T / 4)];
        const float w = wy[3 + k];
        a.x = fmaf(w, v.x, a.x); a.y = fmaf(w, v.y, a.y); a.z = fmaf(w, v.z, a.z); a.w = fmaf(w, v.w, a.w);
    }
    if constexpr (LOG_STORE) {
        const float fl = floor[b];
        float4* dst = reinterpret_cast<float4*>(log_prior + (size_t)b * n + (size_t)(Y0 + y) * HW + X0 + x4);
        *dst = make_float4(logf(a.x + fl), logf(a.y + fl), logf(a.z + fl), logf(a.w + fl));
    } else {
        return a;
    }
}
template <int MERGED>
__device__ __forceinline__ void track_blur_store(const float* src, int S, int P, float* mid, const float* wx, const float* wy, int r,
                                                 const float* floor, float* log_prior, int b, int Y0, int X0) {
    track_blur_tile<MERGED, true>(src, S, P, mid, wx, wy, r, floor, log_prior, b, Y0, X0);
}
template <int MERGED>
__device__ __forceinline__ float4 track_blur_passes(const float* src, int S, int P, float* mid, const float* wx, const float* wy, int r) {
    return track_blur_tile<MERGED, false>(src, S, P, mid, wx, wy, r, nullptr, nullptr, 0, 0, 0);
}

}  // namespace ccvpe
