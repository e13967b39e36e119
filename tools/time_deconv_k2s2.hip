// Dev tool (GPU box): step 0 of DESIGN.md 4.28 - deconv_k2s2_kernel (kernels_deconv.hip) alone on filled buffers at the decoder's
// transposed-conv shapes, before anything is wired (profiles/deconv_k2s2_trace_b32_fp32.md).  One hipEvent pair per launch, median and
// minimum of 100 launches after 30.  The parent's launches of the same layers: tools/time_ops.py '(loc|ori)[2-4]\.deconv' 7 32.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/time_deconv_k2s2.hip -o tools/time_deconv_k2s2
//   tools/time_deconv_k2s2                                   the VIGOR shapes of levels 2-4 at batch 8, 16 and 32
//   tools/time_deconv_k2s2 B H Cin in_ld cw ld scored        one shape (H = W; scored 1: channels 1-7 of the input are unused)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../ccvpe_amd/csrc/kernels_deconv.hip"

namespace ccvpe { thread_local unsigned long long g_launches = 0; }
using namespace ccvpe;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

__global__ void fill_kernel(float* p, size_t n, unsigned seed) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned h = (unsigned)i * 2654435761u + seed;
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        p[i] = (float)(h & 0xffff) * (1.f / 32768.f) - 1.f;
    }
}

static void time_shape(const char* name, int B, int H, int Cin, int in_ld, int cw, int ld, int scored) {
    DeconvK2S2Params p{};
    p.B = B; p.H = H; p.W = H; p.Cin = Cin; p.in_ld = in_ld; p.Kpad = (Cin + 31) / 32 * 32; p.ld = ld; p.coff = 0; p.cw = cw;
    std::vector<unsigned char> live(Cin, 1);
    if (scored) for (int c = 1; c < 8 && c < Cin; ++c) live[c] = 0;
    if (!deconv_k2s2_prepare(p, live.data())) { printf("%-12s B %2d: the kernel does not take Cin %d, cw %d\n", name, B, Cin, cw); return; }
    const size_t nx = (size_t)B * H * H * in_ld, nw = (size_t)4 * cw * p.Kpad, no = (size_t)4 * B * H * H * ld;
    float *x, *w, *b, *o;
    CHECK(hipMalloc(&x, nx * 4)); CHECK(hipMalloc(&w, nw * 4)); CHECK(hipMalloc(&b, (size_t)4 * cw * 4)); CHECK(hipMalloc(&o, no * 4));
    fill_kernel<<<1024, 256>>>(x, nx, 1u);
    fill_kernel<<<256, 256>>>(w, nw, 2u);
    fill_kernel<<<4, 256>>>(b, (size_t)4 * cw, 3u);
    CHECK(hipMemset(o, 0, no * 4));
    p.x = x; p.wpk = w; p.bias = b; p.out = o;
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    std::vector<float> t;
    for (int i = -30; i < 100; ++i) {
        CHECK(hipEventRecord(e0, nullptr));
        launch_deconv_k2s2(p, nullptr);
        CHECK(hipEventRecord(e1, nullptr));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipGetLastError());
        float ms = 0.f;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (i >= 0) t.push_back(ms * 1e3f);
    }
    std::sort(t.begin(), t.end());
    const double mb = ((double)nx * (p.taps == 2 ? 2 : 1) + (double)B * H * H * 4 * cw) * 4e-6;
    printf("%-12s B %2d  rows %7d  Cin %3d (%2d steps of 16)  cw %2d  %d-tap : median %7.1f us  min %7.1f us  %6.1f MB  %5.2f TB/s\n", name, B, B * H * H, Cin,
           p.ngroups / 4, cw, p.taps, t[t.size() / 2], t[0], mb, mb / t[t.size() / 2]);
    CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
    CHECK(hipFree(x)); CHECK(hipFree(w)); CHECK(hipFree(b)); CHECK(hipFree(o));
}

int main(int argc, char** argv) {
    if (argc >= 8) { time_shape("shape", atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7])); return 0; }
    for (int B : {32, 16, 8}) {
        time_shape("loc2.deconv", B, 128, 88, 88, 48, 64, 1);
        time_shape("ori2.deconv", B, 128, 64, 64, 32, 48, 0);
        time_shape("loc3.deconv", B, 64, 168, 168, 80, 104, 1);
        time_shape("ori3.deconv", B, 64, 128, 128, 64, 88, 0);
        time_shape("loc4.deconv", B, 32, 328, 328, 160, 200, 1);
        time_shape("ori4.deconv", B, 32, 256, 256, 128, 168, 0);
    }
    return 0;
}
