// The body of k_conv1_bf16_img (conv1_bf16_img.hpp) over `a`: the kernel's Conv1Args, or a member's entry of a group's device array read
// in place (k_conv1_img_members, conv_group.hpp).  blockIdx.x / gridDim.x: the workgroup and the workgroups of ONE conv1 forward of a.nz instances.
// (no include guard: the text of ONE kernel body, included where the kernel and its group entry stand - the standalone kernel
// compiles the very token sequence it always had, so its registers, LDS and schedule do not move; a __device__ __forceinline__ body
// behind a wrapper moved 50 instantiations of the three units that run these kernels, conv1's weight gradient into scratch)
    C1_TP(0);
    constexpr int PV = c1_plane_vecs(NS), KS = 4 * NS, IMG = NS * 7056, IMG16 = IMG / 16, NW = NT / 64;
    __shared__ uint4 wl[3 * PV];                 // three bf16 weight planes in fragment order
    __shared__ uint4 img[IPW * IMG16 * 2];       // the pass's images as bf16, [image][c][84][84]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int z = blockIdx.x % a.nz, wg = blockIdx.x / a.nz, nwg = gridDim.x / a.nz;
    const int i = lane & 31, h = lane >> 5;
    const int B = a.M / 400;                     // (M = B * 400 always)
    const uint8_t* x = a.x[z];

    constexpr int LPT = (IPW * IMG16 + NT - 1) / NT;   // 16-byte image loads per thread and pass
    int img0 = wg * IPW;
    // the first pass's images: every load in flight while the weights are split (unconditional, clamped: a predicated element would
    // keep the whole array out of registers)
    uint4 stage[LPT];
    const int n16_first = img0 < B ? min(IPW, B - img0) * IMG16 : 0;
    {
        const uint4* src = reinterpret_cast<const uint4*>(x + (size_t)(img0 < B ? img0 : 0) * IMG);
#pragma unroll
        for (int k = 0; k < LPT; ++k) { const int t = tid + NT * k; stage[k] = src[t < n16_first ? t : 0]; }
    }
    {
        // weight split: all of a thread's 8 * WPT loads are in flight before the first one is used (one round trip, not WPT)
        constexpr int WPT = (PV + NT - 1) / NT;
        const float* w1 = a.w1[z];
        float wv[WPT][8];
#pragma unroll
        for (int q = 0; q < WPT; ++q) {
            int t = tid + NT * q;
            t = t < PV ? t : PV - 1;
            const int n = t & 31, hh = (t >> 5) & 1, sx = t >> 6;
#pragma unroll
            for (int j = 0; j < 8; ++j) wv[q][j] = w1[(size_t)(16 * sx + 8 * hh + j) * 32 + n];
        }
#pragma unroll
        for (int q = 0; q < WPT; ++q) {
            const int t = tid + NT * q;
            uint32_t hi[8], mid[8], lo[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                hi[j] = __float_as_uint(wv[q][j]) & 0xffff0000u;
                const float r1 = wv[q][j] - __uint_as_float(hi[j]);     // exact
                mid[j] = __float_as_uint(r1) & 0xffff0000u;
                const float r2 = r1 - __uint_as_float(mid[j]);          // exact, <= 8 significant bits
                lo[j] = __float_as_uint(r2) & 0xffff0000u;
            }
            if (t < PV) {
                wl[0 * PV + t] = uint4{(hi[0] >> 16) | hi[1], (hi[2] >> 16) | hi[3], (hi[4] >> 16) | hi[5], (hi[6] >> 16) | hi[7]};
                wl[1 * PV + t] = uint4{(mid[0] >> 16) | mid[1], (mid[2] >> 16) | mid[3], (mid[4] >> 16) | mid[5], (mid[6] >> 16) | mid[7]};
                wl[2 * PV + t] = uint4{(lo[0] >> 16) | lo[1], (lo[2] >> 16) | lo[3], (lo[4] >> 16) | lo[5], (lo[6] >> 16) | lo[7]};
            }
        }
    }
    // bias of this lane's four channel runs [8 q + 4 h, + 4)
    f32x4 bq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) bq[q] = *reinterpret_cast<const f32x4*>(a.bias[z] + 8 * q + 4 * h);
    C1_TP(1);
#pragma unroll
    for (int k = 0; k < LPT; ++k) {
        const int t = tid + NT * k;
        if (t < n16_first) {
            img[2 * t] = __builtin_bit_cast(uint4, u8x8_to_bf16(stage[k].x, stage[k].y));
            img[2 * t + 1] = __builtin_bit_cast(uint4, u8x8_to_bf16(stage[k].z, stage[k].w));
        }
    }
    C1_TP(2);
    __syncthreads();
    C1_TP(3);
    const uint4* wlane = wl + h * 32 + i;        // fragment (plane pl, k-step s) of this lane (output channel i, k half h): wlane[pl * PV + 64 s]

    float* out = a.out[z];
    const uint8_t* imgb = reinterpret_cast<const uint8_t*>(img);
    C1_TP(4);

    for (bool first = true; img0 < B; img0 += nwg * IPW, first = false) {
        const int nimg = min(IPW, B - img0), Mloc = nimg * 400, units = (Mloc + 31) / 32;
        if (!first) {   // more images than workgroup passes: stage the next ones where the last ones were
            __syncthreads();                 // every wave has read its last fragment of the previous pass
            const uint4* src = reinterpret_cast<const uint4*>(x + (size_t)img0 * IMG);
            for (int t = tid; t < nimg * IMG16; t += NT) {
                const uint4 v = src[t];
                img[2 * t] = __builtin_bit_cast(uint4, u8x8_to_bf16(v.x, v.y));
                img[2 * t + 1] = __builtin_bit_cast(uint4, u8x8_to_bf16(v.z, v.w));
            }
            __syncthreads();
        }
        // a unit's fragments: lane = pixel i of the unit, row parity h; k-step s = patch rows 2 (s % 4) + h of channel s / 4
        auto unit_base = [&](int unit) -> const uint8_t* {
            int m = unit * 32 + i;
            m = m < Mloc ? m : Mloc - 1;
            const int bl = m >= 400 ? 1 : 0, rem = m - bl * 400;
            const int oh = rem / 20, ow = rem - oh * 20;
            return imgb + 2 * (bl * IMG + (oh * 4 + h) * 84 + ow * 4);
        };
        auto frag = [&](const uint8_t* p, int s) -> bf16x8 {
            const uint2* q = reinterpret_cast<const uint2*>(p + 2 * ((s >> 2) * 7056 + ((s & 3) * 2) * 84));
            const uint2 lo = q[0], hi = q[1];
            return __builtin_bit_cast(bf16x8, uint4{lo.x, lo.y, hi.x, hi.y});
        };
        auto store_unit = [&](int unit, const f32x16& acc) {   // lane = pixel i, four runs of 4 consecutive channels [8 q + 4 h, + 4)
            const int m = unit * 32 + i;
#ifdef C1_ABL_NOSTORE
            if (m < Mloc && acc[0] == 12345.678f) {
#else
            if (m < Mloc) {
#endif
                float* o = out + ((size_t)img0 * 400 + m) * 32 + 4 * h;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const float t = acc[4 * q + e] * (1.0f / 255.0f) + bq[q][e]; v[e] = t > 0.f ? t : 0.f; }
                    *reinterpret_cast<f32x4*>(o + 8 * q) = v;
                }
            }
        };
        for (int u = wave; u < units; u += NW) {
            const uint8_t* p = unit_base(u);
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            // pixel fragments two k-steps ahead of the MFMAs that use them, weight fragments one (sched_barrier keeps hipcc from hoisting
            // all the reads of a unit: 4 VGPRs each)
            bf16x8 fa = frag(p, 0), fb = frag(p, 1), wa[3], wb[3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) wa[pl] = __builtin_bit_cast(bf16x8, wlane[pl * PV]);
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const bf16x8 fc = s + 2 < KS ? frag(p, s + 2) : fa;
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) wb[pl] = s + 1 < KS ? __builtin_bit_cast(bf16x8, wlane[pl * PV + 64 * (s + 1)]) : wa[pl];
#pragma unroll
                for (int pl = 2; pl >= 0; --pl) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[pl], fa, acc, 0, 0, 0);   // small terms first
                fa = fb; fb = fc;
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) wa[pl] = wb[pl];
                __builtin_amdgcn_sched_barrier(0);
            }
            store_unit(u, acc);
        }
        C1_TP(6);
    }
