// The body of k_conv1_dw_bf16 (conv1_dw_bf16.hpp) behind its start signal, over `a`: the kernel's Conv1DwArgs, or a member's entry of a
// group's device array read in place (k_conv1_dw_members, conv_group.hpp).  blockIdx.x / gridDim.x: the workgroup and the workgroups of ONE weight gradient.
// (no include guard: the text of ONE kernel body, included where the kernel and its group entry stand - the standalone kernel
// compiles the very token sequence it always had, so its registers, LDS and schedule do not move; a __device__ __forceinline__ body
// behind a wrapper moved 50 instantiations of the three units that run these kernels, conv1's weight gradient into scratch)
    C1DW_TP(0);
    constexpr int TASKS = 4 * ((NS + 1) / 2), TPW = (TASKS + 7) / 8;
    // LDS, dynamic (c1dw_lds_bytes): with a static size hipcc sees that only one workgroup fits a CU and spends the whole register file on
    // its two waves per SIMD (218 VGPRs) - registers that a wave of the OTHER queue's kernel needs to share the SIMD in the two-queue
    // schedule of the DQN step (same kernel, 218 instead of <= 168 VGPRs: the step was 4 us slower although the launch was 2.5 us faster)
    extern __shared__ __attribute__((aligned(16))) uint8_t c1dw_lds[];
    uint16_t* planes = reinterpret_cast<uint16_t*>(c1dw_lds);                                  // [3][32][C1DW_LDM] bf16, 78 336 B
    // the image, [c][84][88] u8: row stride 22 dwords and frame stride 1 872 = 16 (mod 32) dwords put the 2 channels x 8 rows x 2 columns
    // a half wave's ds_read2_b32 touches into 32 different banks (the batch's 21-dword rows would be 2-way conflicts: the k loop is LDS-bound)
    uint32_t* ximg_l = reinterpret_cast<uint32_t*>(c1dw_lds + 3 * 32 * C1DW_LDM * 2);          // NS * C1DW_CH bytes
    float (*sred)[32] = reinterpret_cast<float (*)[32]>(c1dw_lds + 3 * 32 * C1DW_LDM * 2 + NS * C1DW_CH);   // [16][32]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, g = lane >> 5;
    const int pn = tid & 31, pmg = tid >> 5;                      // prologue role: column n, quad group (16 groups)
    const int phase = wave & 3;

    f32x16 acc[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float bsum = 0.f;

    // per-lane A geometry: row i of a tile = (channel 2 pair + i / 16, kh = (i / 2) % 8, kw = phase + 4 (i % 2))
    int c_of[TPW], rowoff; bool live[TPW];
    rowoff = ((i >> 1) & 7) * C1DW_ROW + 4 * (i & 1) + g * (40 * C1DW_ROW);   // lane half g: output rows 10 g ... 10 g + 9
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int task = wave + 8 * t;
        live[t] = task < TASKS;
        const int c = 2 * ((live[t] ? task : 0) >> 2) + (i >> 4);
        c_of[t] = c < NS ? c : NS - 1;
    }

    for (int img = blockIdx.x; img < a.B; img += gridDim.x) {
        // the image -> LDS with coalesced 16-byte loads: the fragments of the k loop are strided gathers (2 channels x 8 rows per half
        // wave) - free in LDS, 4 x the cache lines per instruction of the old tiling when they came straight from memory
        constexpr int XPT = (NS * 441 + 511) / 512;
        uint4 xst[XPT];
        {
            const uint4* xg = reinterpret_cast<const uint4*>(a.x + (size_t)img * (NS * 7056));
#pragma unroll
            for (int k = 0; k < XPT; ++k) { const int t = tid + 512 * k; xst[k] = xg[t < NS * 441 ? t : NS * 441 - 1]; }
        }
        // ---- dY block of this image -> three k-major bf16 planes; bias partial sums
        {
            const float* dyb = a.dy + (size_t)img * 400 * 32;
            float s = 0.f;
            // a thread's quads in two batches (4 + 3): every load of a batch is in flight before its first value is split - two memory
            // round trips instead of seven, 16 live registers instead of 28
#pragma unroll
            for (int q0 = 0; q0 < 7; q0 += 4) {
                float y[4][4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int quad = pmg + 16 * (q0 + q);
#pragma unroll
                    for (int j = 0; j < 4; ++j) y[q][j] = (q0 + q < 7 && quad < 100) ? dyb[(size_t)(4 * quad + j) * 32 + pn] : 0.f;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int quad = pmg + 16 * (q0 + q);
                    if (q0 + q < 7 && quad < 100) {
                        uint32_t hi[4], mid[4], lo[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            s += y[q][j];
                            hi[j] = __float_as_uint(y[q][j]) & 0xffff0000u;
                            const float r1 = y[q][j] - __uint_as_float(hi[j]);      // exact
                            mid[j] = __float_as_uint(r1) & 0xffff0000u;
                            const float r2 = r1 - __uint_as_float(mid[j]);          // exact, <= 8 significant bits
                            lo[j] = __float_as_uint(r2) & 0xffff0000u;
                        }
                        const int o = pn * C1DW_LDM + 4 * quad;
                        *reinterpret_cast<uint2*>(&planes[0 * 32 * C1DW_LDM + o]) = uint2{(hi[0] >> 16) | hi[1], (hi[2] >> 16) | hi[3]};
                        *reinterpret_cast<uint2*>(&planes[1 * 32 * C1DW_LDM + o]) = uint2{(mid[0] >> 16) | mid[1], (mid[2] >> 16) | mid[3]};
                        *reinterpret_cast<uint2*>(&planes[2 * 32 * C1DW_LDM + o]) = uint2{(lo[0] >> 16) | lo[1], (lo[2] >> 16) | lo[3]};
                    }
                }
            }
            sred[pmg][pn] = s;
        }
#pragma unroll
        for (int k = 0; k < XPT; ++k) {
            const int t = tid + 512 * k;
            if (t < NS * 441) {
                const uint32_t w[4] = {xst[k].x, xst[k].y, xst[k].z, xst[k].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int d = 4 * t + e, c = d / 1764, rem = d - c * 1764, r = rem / 21;   // dword d of the packed image -> (frame, row, column)
                    ximg_l[c * (C1DW_CH / 4) + r * (C1DW_ROW / 4) + (rem - r * 21)] = w[e];
                }
            }
        }
        __syncthreads();
        C1DW_TP(1);
        if (tid < 32) {
            float t = sred[0][tid];
#pragma unroll
            for (int k = 1; k < 16; ++k) t += sred[k][tid];
            bsum += t;
        }

        // ---- 25 k-steps of 16 positions, phase-specialised (wave-uniform branch)
        const uint8_t* src[TPW];
        U32x4A4 ring[TPW][C1DW_PF + 1][2];
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            src[t] = reinterpret_cast<const uint8_t*>(ximg_l) + c_of[t] * C1DW_CH + rowoff;
#pragma unroll
            for (int s0 = 0; s0 < C1DW_PF; ++s0) c1dw_load_step(src[t], s0, g, ring[t][s0]);
        }
        if (live[0]) {   // (a wave without a first task has none: tasks are dealt in order)
            if (phase == 0) c1dw_steps<0, TPW>(src, ring, planes, i, g, acc);
            else if (phase == 1) c1dw_steps<1, TPW>(src, ring, planes, i, g, acc);
            else if (phase == 2) c1dw_steps<2, TPW>(src, ring, planes, i, g, acc);
            else c1dw_steps<3, TPW>(src, ring, planes, i, g, acc);
        }
        C1DW_TP(2);
        __syncthreads();   // planes / sred are rewritten by the next image
    }

    float* part = a.part + (size_t)blockIdx.x * a.part_stride;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        if (!live[t]) continue;   // (wave-uniform)
        const int pair = (wave + 8 * t) >> 2;
        // (sixteen dword stores per lane, each a full 128-byte row per half wave; the transposed accumulator - four 16-byte stores of
        // 32-byte row segments - was measured: 2.1 us instead of 1.6 for this epilogue)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * g;                  // row of the tile -> (channel, kh, kw) -> k = (c, kh, kw)
            const int c = 2 * pair + (row >> 4), kh = (row >> 1) & 7, kw = phase + 4 * (row & 1);
            if (c < NS) part[(size_t)(c * 64 + kh * 8 + kw) * 32 + i] = acc[t][r];
        }
    }
    if (tid < 32) part[64 * NS * 32 + tid] = bsum;
    C1DW_TP(3);
