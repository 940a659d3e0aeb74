// Probe: conv2 + conv3 forward of the split-arithmetic DQN step, one k_igemm_b3 launch per layer against the fused per-image launch
// (border_amd/csrc/fwd_c23_b3.hpp): bit comparison of a2 and a3 (must be 0 differing words) and launch times at nz = 1 (the split
// schedule of the step) and nz = 2, back to back and with a1 rewritten before every launch (as conv1 does in the step).
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Iborder_amd/csrc tools/probes/fwd_c23_probe.hip -o tools/probes/fwd_c23_probe.bin
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fwd_c23_b3.hpp"

using namespace bdr;
#define CK(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e__), __LINE__); return 1; } } while (0)

static std::vector<float> host_rand(size_t n, float lo, float hi, unsigned seed)
{
    std::vector<float> h(n);
    unsigned s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < n; ++i) { s = s * 1664525u + 1013904223u; h[i] = lo + (hi - lo) * ((s >> 8) * (1.0f / 16777216.0f)); }
    return h;
}
__global__ void k_copy(const uint4* s, uint4* d, size_t n) { size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; if (i < n) d[i] = s[i]; }

int main(int argc, char** argv)
{
    const int B = argc > 1 ? atoi(argv[1]) : 256;
    const size_t n1 = (size_t)B * 400 * 32, n2 = (size_t)B * 81 * 64, n3 = (size_t)B * 49 * 64;
    FwdB3Args p2{}, p3{};
    FwdC23Args fu{};
    float *a1[2], *shadow[2], *a2p[2], *a3p[2], *a2f[2], *a3f[2];
    for (int z = 0; z < 2; ++z) {
        // a1 as conv1 leaves it: post-ReLU, about half of it zero
        std::vector<float> h1 = host_rand(n1, -1.f, 1.f, 11 + z);
        for (auto& v : h1) v = v > 0.f ? v : 0.f;
        const std::vector<float> w2 = host_rand(512 * 64, -0.06f, 0.06f, 21 + z), w3 = host_rand(576 * 64, -0.06f, 0.06f, 31 + z);
        const std::vector<float> b2 = host_rand(64, -0.1f, 0.1f, 41 + z), b3 = host_rand(64, -0.1f, 0.1f, 51 + z);
        float *dw2, *dw3, *db2, *db3; uint16_t* pl;
        CK(hipMalloc(&a1[z], n1 * 4)); CK(hipMalloc(&shadow[z], n1 * 4));
        CK(hipMemcpy(a1[z], h1.data(), n1 * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(shadow[z], h1.data(), n1 * 4, hipMemcpyHostToDevice));
        CK(hipMalloc(&dw2, w2.size() * 4)); CK(hipMalloc(&dw3, w3.size() * 4)); CK(hipMalloc(&db2, 256)); CK(hipMalloc(&db3, 256));
        CK(hipMemcpy(dw2, w2.data(), w2.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dw3, w3.data(), w3.size() * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(db2, b2.data(), 256, hipMemcpyHostToDevice)); CK(hipMemcpy(db3, b3.data(), 256, hipMemcpyHostToDevice));
        CK(hipMalloc(&pl, CPL_U16 * 2));
        hipLaunchKernelGGL(k_conv_planes, dim3((512 * 64 + 576 * 64 + 255) / 256), dim3(256), 0, 0, dw2, dw3, pl);
        CK(hipMalloc(&a2p[z], n2 * 4)); CK(hipMalloc(&a3p[z], n3 * 4)); CK(hipMalloc(&a2f[z], n2 * 4)); CK(hipMalloc(&a3f[z], n3 * 4));
        p2.x[z] = a1[z]; p2.w[z] = dw2; p2.bias[z] = db2; p2.out[z] = a2p[z]; p2.wpl[z] = pl + CPL_W2;
        p3.x[z] = a2p[z]; p3.w[z] = dw3; p3.bias[z] = db3; p3.out[z] = a3p[z]; p3.wpl[z] = pl + CPL_W3;
        fu.a1[z] = a1[z]; fu.cpl[z] = pl; fu.b2[z] = db2; fu.b3[z] = db3; fu.a2[z] = a2f[z]; fu.a3[z] = a3f[z];
    }
    p2.M = B * 81; p3.M = B * 49;
    CK(hipDeviceSynchronize());
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    auto pair = [&](int nz) -> hipError_t {
        hipError_t e = launch_igemm_b3<FwdC2B3, 6>(0, dim3(m_tiles<FwdC2B3>(p2.M) * n_tiles<FwdC2B3>(), 1, nz), p2);
        return e != hipSuccess ? e : launch_igemm_b3<FwdC3B3, 6>(0, dim3(m_tiles<FwdC3B3>(p3.M) * n_tiles<FwdC3B3>(), 1, nz), p3);
    };
    auto fused = [&](int nz) -> hipError_t { return launch_fwd_c23_b3(0, B, nz, fu); };
    for (int nz = 1; nz <= 2; ++nz) {
        for (int z = 0; z < nz; ++z) {
            CK(hipMemset(a2p[z], 0xff, n2 * 4)); CK(hipMemset(a3p[z], 0xff, n3 * 4)); CK(hipMemset(a2f[z], 0x7f, n2 * 4)); CK(hipMemset(a3f[z], 0x7f, n3 * 4));
        }
        CK(pair(nz)); CK(fused(nz));
        CK(hipDeviceSynchronize());
        size_t d2 = 0, d3 = 0, zero2 = 0, zero3 = 0;
        for (int z = 0; z < nz; ++z) {
            std::vector<uint32_t> x(n2), y(n2);
            CK(hipMemcpy(x.data(), a2p[z], n2 * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(y.data(), a2f[z], n2 * 4, hipMemcpyDeviceToHost));
            for (size_t k = 0; k < n2; ++k) { d2 += x[k] != y[k]; zero2 += x[k] == 0; }
            x.resize(n3); y.resize(n3);
            CK(hipMemcpy(x.data(), a3p[z], n3 * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(y.data(), a3f[z], n3 * 4, hipMemcpyDeviceToHost));
            for (size_t k = 0; k < n3; ++k) { d3 += x[k] != y[k]; zero3 += x[k] == 0; }
        }
        printf("nz=%d B=%d: a2 %zu differing words of %zu (%zu zero), a3 %zu differing words of %zu (%zu zero)\n", nz, B, d2, n2 * nz, zero2, d3, n3 * nz, zero3);
        for (int form = 0; form < 2; ++form) {
            const char* names[2] = {"two launches ", "fused launch "};
            auto go = [&]() -> hipError_t { return form == 0 ? pair(nz) : fused(nz); };
            float tot = 0, mn = 1e9f;
            for (int k = 0; k < 25; ++k) {   // cold input: a1 rewritten before each launch, as conv1 does
                for (int z = 0; z < nz; ++z) hipLaunchKernelGGL(k_copy, dim3((unsigned)((n1 / 4 + 255) / 256)), dim3(256), 0, 0, (const uint4*)shadow[z], (uint4*)a1[z], n1 / 4);
                CK(hipEventRecord(e0));
                CK(go());
                CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
                float ms; CK(hipEventElapsedTime(&ms, e0, e1)); if (k >= 5) { tot += ms; mn = std::min(mn, ms); }
            }
            printf("  %s rewritten a1: %.2f us avg, %.2f min\n", names[form], tot / 20 * 1000, mn * 1000);
            CK(hipEventRecord(e0));
            for (int k = 0; k < 20; ++k) CK(go());
            CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            printf("  %s back to back: %.2f us per form\n", names[form], ms / 20 * 1000);
        }
    }
    return 0;
}
