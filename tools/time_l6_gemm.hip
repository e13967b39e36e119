// Dev tool (GPU box): would a 3x3 layer of the 16 x 16 level-6 map pay in split Winograd form F(4x4,3x3) on the grouped fp32 GEMM of
// kernels_level6.hip (profiles/level6_split_trace_b32_fp32.md)?  Times level6_gemm_kernel alone on filled buffers at
// any (groups, rows, N, Kc) and tile height, and - 36 groups - the split form's two launches around it (split6_transform, split6_inverse).
// One hipEvent pair per launch, median and minimum of `iters` launches after `warm` warm-up launches.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize tools/time_l6_gemm.hip -o tools/time_l6_gemm
//   tools/time_l6_gemm                              the shapes of the profile, 100 launches after 30
//   tools/time_l6_gemm groups rows N Kc [bm]        one shape (N and Kc are rounded up to 128 and 32; bm 128 / 64 / 32, default: the
//                                                   library's rule - level6_rows, 36 groups: split6_rows)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>
#include "../ccvpe_amd/csrc/kernels_level6.hip"

namespace ccvpe { thread_local unsigned long long g_launches = 0; }
using namespace ccvpe;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

static int g_warm = 30, g_iters = 100;

__global__ void fill_kernel(float* p, size_t n, unsigned seed) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned h = (unsigned)i * 2654435761u + seed;
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        p[i] = (float)(h & 0xffff) * (1.f / 32768.f) - 1.f;
    }
}

// launch_level6_gemm with the tile height of p.bm, whatever rule chose it
static void gemm(const Level6Params& p) {
    if (p.bm == 128) launch_gemm_t<128, 2, 2>(p, nullptr);
    else if (p.bm == 64) launch_gemm_t<64, 2, 2>(p, nullptr);
    else launch_gemm_t<32, 1, 4>(p, nullptr);
}

static void time_it(const std::function<void()>& fn, float& median, float& best) {
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    std::vector<float> t;
    for (int i = -g_warm; i < g_iters; ++i) {
        CHECK(hipEventRecord(e0, nullptr));
        fn();
        CHECK(hipEventRecord(e1, nullptr));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipGetLastError());
        float ms = 0.f;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (i >= 0) t.push_back(ms * 1e3f);
    }
    std::sort(t.begin(), t.end());
    median = t[t.size() / 2]; best = t[0];
    CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
}

static void time_shape(int groups, int rows, int N, int Kc, int bm) {
    Level6Params p{};
    p.wm = 4; p.groups = groups; p.N = N; p.Npad = (N + 127) / 128 * 128; p.Kc = (Kc + 31) / 32 * 32; p.K = p.Kc;
    if (groups == 36 && rows % 16 == 0) split6_rows(rows / 16, &p.bm);
    else p.bm = rows > 64 ? 128 : rows > 32 ? 64 : 32;   // level6_rows
    if (bm) p.bm = bm;
    p.R = (rows + p.bm - 1) / p.bm * p.bm;
    const size_t nv = (size_t)groups * p.R * p.Kc, nw = (size_t)groups * p.Npad * p.Kc, nm = (size_t)groups * p.R * p.N;
    float *v, *w, *m;
    CHECK(hipMalloc(&v, nv * 4)); CHECK(hipMalloc(&w, nw * 4)); CHECK(hipMalloc(&m, nm * 4));
    fill_kernel<<<1024, 256>>>(v, nv, 1u);
    fill_kernel<<<1024, 256>>>(w, nw, 2u);
    CHECK(hipMemset(m, 0, nm * 4));
    p.v = v; p.wc = w; p.mp = m;
    float med, best;
    time_it([&] { gemm(p); }, med, best);
    const double gflop = 2.0 * groups * p.R * (double)p.Npad * p.Kc * 1e-9;
    printf("gemm      groups %3d  R %4d (bm %3d)  N %4d / %4d  Kc %4d : median %7.1f us  min %7.1f us  %6.2f GFLOP issued  %6.1f TFLOP/s  (%d workgroups)\n", groups,
           p.R, p.bm, p.N, p.Npad, p.Kc, med, best, gflop, gflop / med * 1e3, groups * (p.R / p.bm) * (p.Npad / 128));
    if (groups == 36 && rows % 16 == 0 && Kc % 4 == 0 && N % 4 == 0) {   // the split form's own launches around it
        Split6Params q{};
        q.B = rows / 16; q.C = Kc; q.Kc = p.Kc; q.N = N; q.Npad = p.Npad; q.R = p.R; q.bm = p.bm;
        const size_t nx = (size_t)q.B * 256 * Kc, no = (size_t)q.B * 256 * N;
        float *x, *o, *bias;
        CHECK(hipMalloc(&x, nx * 4)); CHECK(hipMalloc(&o, no * 4)); CHECK(hipMalloc(&bias, (size_t)N * 4));
        fill_kernel<<<1024, 256>>>(x, nx, 3u);
        fill_kernel<<<4, 256>>>(bias, (size_t)N, 4u);
        q.x = x; q.x_ld = Kc; q.x_coff = 0; q.v = v; q.wc = w; q.mp = m; q.bias = bias; q.relu = 0; q.out = o; q.out_ld = N; q.out_coff = 0;
        time_it([&] { launch_split6_transform(q, nullptr); }, med, best);
        printf("transform B %d C %d: median %7.1f us  min %7.1f us  (%.1f MB)\n", q.B, q.C, med, best, (nx + nv) * 4e-6);
        time_it([&] { launch_split6_inverse(q, nullptr); }, med, best);
        printf("inverse   B %d N %d: median %7.1f us  min %7.1f us  (%.1f MB)\n", q.B, q.N, med, best, (no + nm) * 4e-6);
        time_it([&] { launch_split6_transform(q, nullptr); gemm(p); launch_split6_inverse(q, nullptr); }, med, best);
        printf("all three            : median %7.1f us  min %7.1f us\n", med, best);
        CHECK(hipFree(x)); CHECK(hipFree(o)); CHECK(hipFree(bias));
    }
    CHECK(hipFree(v)); CHECK(hipFree(w)); CHECK(hipFree(m));
}

int main(int argc, char** argv) {
    if (argc >= 5) { time_shape(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), argc > 5 ? atoi(argv[5]) : 0); return 0; }
    time_shape(100, 128, 640, 1344, 0);   // the composed launch: the rate the issue assumes
    time_shape(36, 512, 640, 640, 128);   // conv6.2 in split form, the composed launch's tile height
    time_shape(36, 512, 640, 320, 128);   // the skip half of conv6.0
    time_shape(100, 128, 640, 1344, 0);   // ... again, behind them: the clocks of the run
    // what the two differences from the composed launch cost, one at a time
    time_shape(100, 128, 640, 640, 0);    // the depth alone: 500 workgroups, 20 k-tiles
    time_shape(100, 128, 640, 320, 0);    // 10 k-tiles
    time_shape(36, 512, 640, 1344, 128);  // the grid alone: 720 workgroups on 256 CUs, 42 k-tiles
    time_shape(36, 512, 640, 640, 64);    // 64-row tiles: 1440 workgroups
    time_shape(36, 512, 640, 320, 64);
    return 0;
}
