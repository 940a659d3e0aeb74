// conv2 / conv3 input-gradient kernels of the product (FP32 MFMA) with parts switched off (igemm.hpp BDR_IGEMM_ABL): where does the time go?
// Build (one binary per ablation): hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Iborder_amd/csrc -DBDR_IGEMM_ABL=<n> tools/probes/dx_abl.hip -o tools/probes/dx_abl_<n>.bin
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cnn_layers.hpp"

using namespace bdr;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)
#ifndef BDR_IGEMM_ABL
#define BDR_IGEMM_ABL 0
#endif

static float* dev_rand(size_t n, float lo, float hi, unsigned seed)
{
    std::vector<float> h(n);
    unsigned s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < n; ++i) { s = s * 1664525u + 1013904223u; h[i] = lo + (hi - lo) * ((s >> 8) * (1.0f / 16777216.0f)); }
    float* d; CK(hipMalloc(&d, n * 4)); CK(hipMemcpy(d, h.data(), n * 4, hipMemcpyHostToDevice));
    return d;
}
template <class F>
static double time_us(F f)
{
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int i = 0; i < 5; ++i) f();
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0, 0));
    for (int i = 0; i < 100; ++i) f();
    CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    return ms * 1000.0 / 100;
}

int main()
{
    const int B = 256;
    const size_t n1 = (size_t)B * 400 * 32, n2 = (size_t)B * 81 * 64, n3 = (size_t)B * 49 * 64;
    float* w2 = dev_rand(512 * 64, -0.05f, 0.05f, 2);
    float* w3 = dev_rand(576 * 64, -0.05f, 0.05f, 4);
    float* dy2 = dev_rand(n2, -1.f, 1.f, 8);
    float* dy3 = dev_rand(n3, -1.f, 1.f, 6);
    float* mask1 = dev_rand(n1, -1.f, 1.f, 9);
    float* mask2 = dev_rand(n2, -1.f, 1.f, 7);
    float *dx1, *dx2; CK(hipMalloc(&dx1, n1 * 4)); CK(hipMalloc(&dx2, n2 * 4));
    DxArgs d2{dy2, w2, mask1, dx1, B * 100, nullptr, 0};
    DxArgs d3{dy3, w3, mask2, dx2, B * 81, nullptr, 0};
    const char* what[8] = {"full", "no k loop", "no stores", "no k loop, no stores", "no mask loads", "no k loop, no mask loads", "no stores, no mask loads", "launch + row maps only"};
    printf("ablation %d (%s)\n", BDR_IGEMM_ABL, what[BDR_IGEMM_ABL & 7]);
    printf("  conv2 dX merged classes, 64 x 128 tiles, 400 workgroups : %7.2f us\n", time_us([&] { CK((launch_igemm<DxC2M, 1>(0, dim3(m_tiles<DxC2M>(d2.M) * n_tiles<DxC2M>(), 1, 1), d2))); }));
    printf("  conv3 dX position classes, 2 teams                      : %7.2f us\n",
           time_us([&] { CK((launch_igemm<DxC3Pos, 2>(0, dxc3_pos_grid<DxC3Pos>(B), d3))); }));
    // one workgroup per CU for the position-class kernel: extra dynamic LDS so that a second workgroup does not fit beside the first (the
    // 68 workgroups behind the first 256 then start where a SHORT workgroup has finished, not beside an interior position's 9 iterations)
    for (unsigned extra : {0u, 8u << 10, 16u << 10, 24u << 10}) {
        const dim3 g = dxc3_pos_grid<DxC3Pos>(B);
        printf("  conv3 dX position classes, 2 teams, +%2u KB dynamic LDS   : %7.2f us\n", extra >> 10, time_us([&] {
            hipExtLaunchKernelGGL((k_igemm<DxC3Pos, 2>), g, dim3(64 * DxC3Pos::WM * DxC3Pos::WN * 2), extra, 0, nullptr, nullptr, 0, d3);
            CK(hipGetLastError()); }));
    }
    // conv3 dX back to back: the plain two-team loop, its last step peeled (k_igemm's PEEL), ADxS1PosLean's addressing, both (the product's
    // launch), and one team (one chain over all k-tiles: other roundings than two teams); l1 dX with the peeled loop.  Every two-team form must give the first one's words.
    auto same_bits = [&](float* out, size_t n, auto f_old, auto f_new) {
        std::vector<unsigned> a(n), b(n);
        CK(hipMemset(out, 0xff, n * 4)); f_old(); CK(hipMemcpy(a.data(), out, n * 4, hipMemcpyDeviceToHost));
        CK(hipMemset(out, 0xff, n * 4)); f_new(); CK(hipMemcpy(b.data(), out, n * 4, hipMemcpyDeviceToHost));
        size_t bad = 0;
        for (size_t i = 0; i < n; ++i) bad += a[i] != b[i];
        return bad;
    };
    const dim3 g3 = dxc3_pos_grid<DxC3Pos>(B);
    auto c3_t2 = [&] { CK((launch_igemm<DxC3Pos, 2>(0, g3, d3))); };
    auto c3_pl = [&] { CK((launch_igemm<DxC3Pos, 2, true>(0, g3, d3))); };
    auto c3_ln = [&] { CK((launch_igemm<DxC3PosL, 2>(0, g3, d3))); };
    auto c3_lp = [&] { CK((launch_igemm<DxC3PosL, 2, true>(0, g3, d3))); };
    auto c3_t1 = [&] { CK((launch_igemm<DxC3Pos, 1>(0, g3, d3))); };
    auto c3_l1 = [&] { CK((launch_igemm<DxC3PosL, 1>(0, g3, d3))); };
    printf("  conv3 dX, 2 teams                                       : %7.2f us\n", time_us(c3_t2));
    printf("  conv3 dX, 2 teams, last step peeled                     : %7.2f us   (%zu words differ)\n", time_us(c3_pl), same_bits(dx2, n2, c3_t2, c3_pl));
    printf("  conv3 dX, 2 teams, lean addressing                      : %7.2f us   (%zu words differ)\n", time_us(c3_ln), same_bits(dx2, n2, c3_t2, c3_ln));
    printf("  conv3 dX, 2 teams, last step peeled, lean addressing    : %7.2f us   (%zu words differ)\n", time_us(c3_lp), same_bits(dx2, n2, c3_t2, c3_lp));
    printf("  conv3 dX, 1 team                                        : %7.2f us\n", time_us(c3_t1));
    printf("  conv3 dX, 1 team, lean addressing                       : %7.2f us   (%zu words differ from 1 team)\n", time_us(c3_l1), same_bits(dx2, n2, c3_t1, c3_l1));
    float* dh1 = dev_rand((size_t)B * 512, -1.f, 1.f, 10);
    float* w4 = dev_rand((size_t)3136 * 512, -0.05f, 0.05f, 11);
    float* mask3 = dev_rand(n3, -1.f, 1.f, 12);
    float* dx3; CK(hipMalloc(&dx3, n3 * 4));
    DxArgs d4{dh1, w4, mask3, dx3, B, nullptr, 0};
    const dim3 g4((m_tiles<DxL1>(B) * n_tiles<DxL1>() + 7) / 8 * 8, 1, 1);
    auto l1_t2 = [&] { CK((launch_igemm<DxL1, 2>(0, g4, d4))); };
    auto l1_pl = [&] { CK((launch_igemm<DxL1, 2, true>(0, g4, d4))); };
    printf("  l1 dX, 2 teams                                          : %7.2f us\n", time_us(l1_t2));
    printf("  l1 dX, 2 teams, last step peeled                        : %7.2f us   (%zu words differ)\n", time_us(l1_pl), same_bits(dx3, n3, l1_t2, l1_pl));
    return 0;
}
