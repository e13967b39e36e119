// Heading prior (the parameters are defined in kernels.h): information about the heading coming IN.  The orientation
// field is the network's p(heading | position), so a prior over the heading - a table T of nb + 1 log-weights, entry nb for a cell
// without a heading - is a per-cell log-weight T[bin(c_i, s_i)] on the position grid.  heading_prior_map_kernel writes that map (plus a
// position prior, when there is one); every existing prior form then takes it as its log_prior.  heading_predict_kernel is the
// heading-axis twin of track_predict_kernel: the last frame's hist, turned, blurred on the circle, floored, as the next frame's table.
#include "kernels.h"
#include "tail_shared.h"

namespace ccvpe {

// Grid (64 chunks, B), 256 threads.  The query's table goes into LDS (nb + 1 <= 361 floats); per thread four float4 of c, of s and
// (PRIOR) of P, all in flight in one trip, then four float4 stores of comb = T[k] or P + T[k] (one IEEE add), k = the cell's bin by
// heading_reduce_kernel's own expression (tail_shared.h), nb for a cell without a heading.  No atomics, no tickets: every output word
// depends on its own cell and the table only.  Every global address lies inside its tensor whatever the field or the table holds: whole
// chunks, a table index in [0, nb] by construction (heading_bin clamps; min() below for the reader), nb clamped to the table's range.
template <bool PRIOR>
__global__ __launch_bounds__(256) void heading_prior_map_kernel(const HeadingPriorMapParams p) {
    __shared__ float lt[HEADING_MAX_BINS + 1];
    constexpr int n = TAIL_HW * TAIL_HW, per = n / TAIL_CHUNKS;   // 4096: a multiple of 4 x 256
    const int b = blockIdx.y, lo = blockIdx.x * per;
    const int nb = min(max(p.nb, HEADING_MIN_BINS), HEADING_MAX_BINS);
    const float* tb = p.table + (size_t)b * p.table_stride;
    for (int i = threadIdx.x; i <= nb; i += 256) lt[i] = tb[i];
    const float* oc = p.ori + (size_t)b * 2 * n;
    const float* os = oc + n;
    float4 fc[4], fs[4], q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) fc[u] = reinterpret_cast<const float4*>(oc + lo)[threadIdx.x + u * 256];
#pragma unroll
    for (int u = 0; u < 4; ++u) fs[u] = reinterpret_cast<const float4*>(os + lo)[threadIdx.x + u * 256];
    if constexpr (PRIOR) {
        const float* lp = p.prior + (size_t)b * p.prior_stride;
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = reinterpret_cast<const float4*>(lp + lo)[threadIdx.x + u * 256];
    }
    __syncthreads();
    const float scale = (float)nb / 360.f;
    auto cell = [&](float cs, float sn) {
        const int k = heading_valid(cs, sn) ? heading_bin(cs, sn, scale, nb) : nb;
        return lt[min(max(k, 0), nb)];
    };
    float4* out = reinterpret_cast<float4*>(p.out + (size_t)b * n + lo);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        float4 t = make_float4(cell(fc[u].x, fs[u].x), cell(fc[u].y, fs[u].y), cell(fc[u].z, fs[u].z), cell(fc[u].w, fs[u].w));
        if constexpr (PRIOR) { t.x = q[u].x + t.x; t.y = q[u].y + t.y; t.z = q[u].z + t.z; t.w = q[u].w + t.w; }
        out[threadIdx.x + u * 256] = t;
    }
}

void launch_heading_prior_map(const HeadingPriorMapParams& p, hipStream_t s) {
    if (p.prior) CCVPE_LAUNCH(heading_prior_map_kernel<true>, dim3(TAIL_CHUNKS, p.B), dim3(256), 0, s, p);
    else CCVPE_LAUNCH(heading_prior_map_kernel<false>, dim3(TAIL_CHUNKS, p.B), dim3(256), 0, s, p);
}

// Grid (B), 256 threads: one workgroup per query, everything on the circle of nb bins in LDS.
//     u    = (double)b - (double)turn_deg / (360.0 / nb),  i0 = floor(u),  f = (float)(u - i0)          rounded once
//     s(b) = (1.f - f) * hist[i0 mod nb] + f * hist[(i0 + 1) mod nb]       f == 0 weighs the one source bin with exactly 1
//     c(b) = sum over j = -r .. r, ascending, of fmaf(t[|j|], s[(b + j) mod nb], c)                       2r + 1 fused multiply-adds
//     out[b] = logf(c(b) + floor),  out[nb] = logf((float)(float64 sum of c in index order / nb) + floor)
// The integer part is clamped to +-2^30 before it is converted (fmax returns the clamp for NaN, as in track_predict_affine_kernel) and
// reduced modulo nb, so no turn - NaN and infinities included - moves a read outside hist; such a turn gives NaN weights, i.e. a NaN row.
__global__ __launch_bounds__(256) void heading_predict_kernel(const HeadingPredictParams p) {
    __shared__ float sh[HEADING_MAX_BINS];            // the turned histogram s
    __shared__ float sc[HEADING_MAX_BINS];            // the blurred one c
    __shared__ float st[TRACK_MAX_R + 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nb = min(max(p.nb, HEADING_MIN_BINS), HEADING_MAX_BINS);
    const int r = min(min(max(p.radius, 0), TRACK_MAX_R), (nb - 1) / 2);
    const float* hist = p.hist + (size_t)b * nb;
    if (tid <= r) st[tid] = p.taps[(size_t)b * p.taps_stride + tid];
    const double shift = (double)p.turn_deg[b] / (360.0 / (double)nb);
    for (int i = tid; i < nb; i += 256) {
        const double u = (double)i - shift;
        const double fl = floor(u);
        const float f = (float)(u - fl);
        const int ic = (int)fmin(fmax(fl, -1073741824.), 1073741824.);
        int i0 = ic % nb;
        if (i0 < 0) i0 += nb;
        const int i1 = i0 + 1 == nb ? 0 : i0 + 1;
        sh[i] = (1.f - f) * hist[i0] + f * hist[i1];
    }
    __syncthreads();
    const float fl = p.floor[b];
    float* out = p.out + (size_t)b * (nb + 1);
    for (int i = tid; i < nb; i += 256) {
        float a = 0.f;
        int k = i - r;
        if (k < 0) k += nb;                           // (2r + 1 <= nb: one wrap either way)
        for (int j = -r; j <= r; ++j) {
            a = fmaf(st[j < 0 ? -j : j], sh[k], a);
            if (++k == nb) k = 0;
        }
        sc[i] = a;
        out[i] = logf(a + fl);
    }
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int i = 0; i < nb; ++i) sum += (double)sc[i];
        out[nb] = logf((float)(sum / (double)nb) + fl);
    }
}

void launch_heading_predict(const HeadingPredictParams& p, hipStream_t s) {
    CCVPE_LAUNCH(heading_predict_kernel, dim3(p.B), dim3(256), 0, s, p);
}

}  // namespace ccvpe
