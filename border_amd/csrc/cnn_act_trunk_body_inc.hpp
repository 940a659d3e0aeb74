// The body of k_cnn_act_trunk (cnn_act_img.hpp) over `a`: the kernel's CnnActTrunkArgs, or the words of one member of a group call
// gathered into a CnnActTrunkArgs in registers (k_cnn_act_trunk_group).  blockIdx.x: the frame stack of a.rows and the row of a.feat.
// (no include guard: the text of ONE kernel body, included where the kernel and its group entry stand - the standalone kernel
// compiles the very token sequence it always had, so its registers, LDS and schedule do not move)
    __shared__ __attribute__((aligned(16))) float s_u[3 * CAI_RED];
    __shared__ __attribute__((aligned(16))) float s_a1[400 * CAI_A1_LD];
    __shared__ __attribute__((aligned(16))) float s_a2[81 * CAI_A2_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;

    // ---- every first operand, requested before anything is waited for
    // conv1: the fragment rows of channel c for this lane (output channel i, k half h): W1[64 c + 16 sl + 8 h + j][i]
    auto load_w1 = [&](int c, float (&w)[4][8]) __attribute__((always_inline)) {
#pragma unroll
        for (int sl = 0; sl < 4; ++sl)
#pragma unroll
            for (int j = 0; j < 8; ++j) w[sl][j] = a.w1[(size_t)(64 * c + 16 * sl + 8 * h + j) * 32 + i];
    };
    // conv2: chunk ch = k-steps 2 ch, 2 ch + 1 of this wave's quarter, both column tiles: W2[128 w + 8 s + 4 h + q][32 nt + i]
    auto load_w2 = [&](int ch, float (&w)[2][2][4]) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int q = 0; q < 4; ++q) w[u][nt][q] = a.w2[(size_t)(128 * wave + 8 * (2 * ch + u) + 4 * h + q) * 64 + 32 * nt + i];
    };
    // conv3: one tap of this wave's column tile: W3[64 tap + 8 s + 4 h + q][32 (w & 1) + i]
    auto load_w3 = [&](int tap, float (&w)[8][4]) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int q = 0; q < 4; ++q) w[s][q] = a.w3[(size_t)(64 * tap + 8 * s + 4 * h + q) * 64 + 32 * (wave & 1) + i];
    };
    float w1n[4][8], w2n[2][2][4], w3n[8][4];
    load_w1(0, w1n);
    f32x4 bq1[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) bq1[q] = *reinterpret_cast<const f32x4*>(a.b1 + 8 * q + 4 * h);
    load_w2(0, w2n);
    load_w3(0, w3n);
    const float b3v = a.b3[32 * (wave & 1) + i];

    // ---- the frame stack -> LDS, as it is (u8)
    {
        const uint8_t* src = a.rows + (size_t)blockIdx.x * a.row_stride;
        if (a.vec16) cai_stage(reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(s_u), a.ns * 441, tid);
        else cai_stage(reinterpret_cast<const uint32_t*>(src), reinterpret_cast<uint32_t*>(s_u), a.ns * 1764, tid);
    }
    __syncthreads();

    // ---- conv1
    {
        const int nu = wave == 0 ? 4 : 3;
        const uint8_t* frb = reinterpret_cast<const uint8_t*>(s_u);
        int poff[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int m = min((wave + 4 * t) * 32 + i, 399), oh = m / 20, ow = m - oh * 20;
            poff[t] = (oh * 4 + h) * 84 + ow * 4;
        }
        f32x16 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        for (int c = 0; c < a.ns; ++c) {
            float wc[4][8];
#pragma unroll
            for (int sl = 0; sl < 4; ++sl)
#pragma unroll
                for (int j = 0; j < 8; ++j) wc[sl][j] = w1n[sl][j];
            if (c + 1 < a.ns) load_w1(c + 1, w1n);
#pragma unroll
            for (int sl = 0; sl < 4; ++sl) {
                uint32_t hi[8], mid[8], lo[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    hi[j] = __float_as_uint(wc[sl][j]) & 0xffff0000u;
                    const float r1 = wc[sl][j] - __uint_as_float(hi[j]);    // exact
                    mid[j] = __float_as_uint(r1) & 0xffff0000u;
                    const float r2 = r1 - __uint_as_float(mid[j]);          // exact, <= 8 significant bits
                    lo[j] = __float_as_uint(r2) & 0xffff0000u;
                }
                bf16x8 wp[3];
                wp[0] = __builtin_bit_cast(bf16x8, uint4{(hi[0] >> 16) | hi[1], (hi[2] >> 16) | hi[3], (hi[4] >> 16) | hi[5], (hi[6] >> 16) | hi[7]});
                wp[1] = __builtin_bit_cast(bf16x8, uint4{(mid[0] >> 16) | mid[1], (mid[2] >> 16) | mid[3], (mid[4] >> 16) | mid[5], (mid[6] >> 16) | mid[7]});
                wp[2] = __builtin_bit_cast(bf16x8, uint4{(lo[0] >> 16) | lo[1], (lo[2] >> 16) | lo[3], (lo[4] >> 16) | lo[5], (lo[6] >> 16) | lo[7]});
                // k-step sl of channel c: patch rows 2 sl + h, eight pixels of the row per lane
                const int so = c * 7056 + (2 * sl) * 84;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (t < nu) {   // wave-uniform
                        const uint32_t* px = reinterpret_cast<const uint32_t*>(frb + poff[t] + so);
                        const bf16x8 fa = u8x8_to_bf16(px[0], px[1]);
#pragma unroll
                        for (int pl = 2; pl >= 0; --pl) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wp[pl], fa, acc[t], 0, 0, 0);   // small terms first
                    }
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int m = (wave + 4 * t) * 32 + i;
            if (t < nu && m < 400) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const float x = acc[t][4 * q + e] * (1.0f / 255.0f) + bq1[q][e]; v[e] = x > 0.f ? x : 0.f; }
                    *reinterpret_cast<f32x4*>(s_a1 + m * CAI_A1_LD + 8 * q + 4 * h) = v;
                }
            }
        }
    }
    __syncthreads();   // a1 is whole; nobody reads the frames any more

    // ---- conv2: this wave's k-quarter (kernel row kh = wave) of all six tiles
    {
        int ab[3];
#pragma unroll
        for (int mt = 0; mt < 3; ++mt) {
            const int m = min(32 * mt + i, 80), oh = m / 9, ow = m - oh * 9;
            ab[mt] = ((2 * oh + wave) * 20 + 2 * ow) * CAI_A1_LD + 4 * h;
        }
        f32x16 acc[3][2];
#pragma unroll
        for (int mt = 0; mt < 3; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
        for (int ch = 0; ch < 8; ++ch) {
            float wc[2][2][4];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int q = 0; q < 4; ++q) wc[u][nt][q] = w2n[u][nt][q];
            if (ch + 1 < 8) load_w2(ch + 1, w2n);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int s = 2 * ch + u, ko = (s >> 2) * CAI_A1_LD + (s & 3) * 8;   // k = 8 s + 4 h: kw = s >> 2, channels (s & 3) 8 + 4 h ...
                f32x4 av[3];
#pragma unroll
                for (int mt = 0; mt < 3; ++mt) av[mt] = *reinterpret_cast<const f32x4*>(s_a1 + ab[mt] + ko);
#pragma unroll
                for (int mt = 0; mt < 3; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt][q], wc[u][nt][q], acc[mt][nt], 0, 0, 0);
            }
        }
        // the quarters meet: wave 0 in a2 itself, waves 1 ... 3 in red (over the frames)
        float* dst = wave == 0 ? s_a2 : s_u + (wave - 1) * CAI_RED;
        const int ld = wave == 0 ? CAI_A2_LD : 64;
#pragma unroll
        for (int mt = 0; mt < 3; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (m < 81) dst[m * ld + 32 * nt + i] = acc[mt][nt][r];
                }
    }
    __syncthreads();
    for (int e = tid; e < CAI_RED; e += 256) {   // one thread per element: ((q0 + q1) + q2) + q3, bias, ReLU
        const int m = e >> 6, n = e & 63;
        float v = ((s_a2[m * CAI_A2_LD + n] + s_u[e]) + s_u[CAI_RED + e]) + s_u[2 * CAI_RED + e];
        v += a.b2[n];
        s_a2[m * CAI_A2_LD + n] = v > 0.f ? v : 0.f;
    }
    __syncthreads();

    // ---- conv3: tile (wave >> 1, wave & 1)
    {
        const int mt = wave >> 1, nt = wave & 1;
        const int mc = min(32 * mt + i, 48), oh = mc / 7, ow = mc - oh * 7;
        const int ab = (oh * 9 + ow) * CAI_A2_LD + 4 * h;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int tap = 0; tap < 9; ++tap) {
            float wc[8][4];
#pragma unroll
            for (int s = 0; s < 8; ++s)
#pragma unroll
                for (int q = 0; q < 4; ++q) wc[s][q] = w3n[s][q];
            if (tap + 1 < 9) load_w3(tap + 1, w3n);
            const int kh = tap / 3, kw = tap - kh * 3, to = ab + (kh * 9 + kw) * CAI_A2_LD;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(s_a2 + to + 8 * s);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q], wc[s][q], acc, 0, 0, 0);
            }
        }
        float* out = a.feat + (size_t)blockIdx.x * 3136 + 32 * nt + i;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * h;
            const float v = acc[r] + b3v;
            if (m < 49) out[m * 64] = v > 0.f ? v : 0.f;
        }
    }
