// The body of k_igemm (igemm.hpp) over `args` (a typename P::Args) for workgroup (IGEMM_BX, IGEMM_BY, IGEMM_BZ) of the GEMM's own grid:
// blockIdx in the standalone kernel, the member's own grid in k_igemm_members (conv_group.hpp).  P, TEAMS, PEEL: the kernel's.
// (no include guard: the text of ONE kernel body, included where the kernel and its group entry stand - the standalone kernel
// compiles the very token sequence it always had, so its registers, LDS and schedule do not move; a __device__ __forceinline__ body
// behind a wrapper moved 50 instantiations of the three units that run these kernels, conv1's weight gradient into scratch)
    using A = typename P::A;
    constexpr int NW = P::WM * P::WN, NT = 64 * NW;          // waves / threads per team
    constexpr int BM = P::WM * P::TM * 32, BN = P::WN * P::TN * 32;
    constexpr int LDB = BN;
    constexpr int APR = BK / A::VEC;                         // staging loads per A row
    static_assert(NT % APR == 0, "thread count must keep the k-quad of a thread fixed across passes");
    constexpr int A_ELEMS = BM * APR;
    constexpr int A_PASSES = (A_ELEMS + NT - 1) / NT;
    constexpr int AV = A::VEC / 4;
    constexpr int B_ELEMS = BK * BN / 4;
    constexpr int B_VECS = (B_ELEMS + NT - 1) / NT;          // f32x4 per thread for the B tile
    static_assert(TEAMS == 1 || TEAMS == 2, "one or two teams");

    // two LDS stages per team: tile t+1 is written while tile t feeds the matrix pipe (one barrier per k-tile)
    constexpr int STAGE = BM * LDA + (P::B_TR ? BN * LDA : BK * LDB);
    static_assert(TEAMS == 1 || 2 * STAGE >= BM * BN, "team reduction buffer must fit one team's stages");
    __shared__ __attribute__((aligned(16))) float smem_all[2 * STAGE * TEAMS];

    const int team = TEAMS == 1 ? 0 : (int)(threadIdx.x / NT);
    float* smem = smem_all + team * 2 * STAGE;
    const int tid = threadIdx.x % NT, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / P::WN, wn = wave % P::WN;
    const int NT_N = P::N(args) / BN;
    const int M = P::M(args);
    // block -> (m-tile, n-tile, instance) map.  Workgroup b runs on XCD b % 8 and every XCD has its own L2, so which tiles
    // share an XCD decides how often an operand crosses the fabric (PMC: l1 forward moved 71.6 MB for 26.5 MB of operands
    // and results with the plain map, every XCD streaming all of A).
    int mt, nt, z = IGEMM_BZ, y = IGEMM_BY;
    if constexpr (xmap_of<P>::value == 3) {
        // split-K slice = XCD: XCD j multiplies k-slice j of every output tile, so each XCD's L2 sees 1/8 of A's columns and 1/8
        // of B's rows exactly once (PMC, round 3: the (instance, n-tile pair) map fetched 38.6 MB for 19.3 MB of operands - every A
        // element crossed the fabric four times).  grid: (8 * m-tiles * n-tiles, 1, instances)
        y = IGEMM_BX & 7;
        const int j = IGEMM_BX >> 3;
        nt = j % NT_N; mt = j / NT_N;
    } else if constexpr (xmap_of<P>::value == 1) {
        // contiguous runs of tiles per XCD, m fastest: the m-tiles of one n-tile (same B columns) meet in one L2
        const int MT = (M + BM - 1) / BM, per = gridDim.x >> 3;   // (flat rows: RPIP == 0)
        const int t = (IGEMM_BX & 7) * per + (IGEMM_BX >> 3);
        if (t >= MT * NT_N) return;
        nt = t / MT; mt = t % MT;
    } else if constexpr (xmap_of<P>::value == 2) {
        // 8 n-tiles, instances in pairs: XCD = (instance parity, pair of n-tiles); each B element is read by one XCD,
        // each A element by four.  grid: (16 * m-tiles, splits, instances / 2)
        const int xcd = IGEMM_BX & 7, j = IGEMM_BX >> 3;
        z = IGEMM_BZ * 2 + (xcd >> 2);
        nt = (xcd & 3) * 2 + (j & 1); mt = j >> 1;
    } else {
        mt = IGEMM_BX / NT_N; nt = IGEMM_BX % NT_N;
    }
    const int m0 = mt * BM, n0 = nt * BN;                    // m0: virtual row

    // per-thread staging coordinates: element e = tid + p*NT of the A tile -> (row e / APR, k-quad e % APR)
    const int a_q = tid % APR, a_r = tid / APR;
    typename A::Row rows[A_PASSES];
#pragma unroll
    for (int p = 0; p < A_PASSES; ++p) {
        int mr;
        const bool ok = vrow_of<P>(args, y, m0 + p * (NT / APR) + a_r, mr);
        rows[p] = A::row(P::a_src(args, z), ok ? mr : M, M);   // invalid rows alias row 0 and are never stored
    }
    const float* w = P::w(args, z, y);

    int kt0, kt1;
    P::kt_range(args, y, kt0, kt1);
    // team g owns k-tiles kt0+g, kt0+g+TEAMS, ...; both teams run the same number of iterations so the
    // workgroup barriers match (the shorter team idles through its last one)
#ifdef BDR_IGEMM_ABL   // (tools/probes/dx_abl.hip) bit 0: no k loop, bit 1: no stores, bit 2: no epilogue operand loads
    constexpr int ABL = BDR_IGEMM_ABL;
#else
    constexpr int ABL = 0;
#endif
    const int iters = (ABL & 1) ? 0 : (kt1 - kt0 + TEAMS - 1) / TEAMS;
    const int my_n = (ABL & 1) ? 0 : (kt0 + team < kt1 ? (kt1 - kt0 - team + TEAMS - 1) / TEAMS : 0);
    auto tile = [&](int it) { return kt0 + team + min(it, max(my_n - 1, 0)) * TEAMS; };   // clamped to my last tile

    // Two register sets: global loads are issued ~2 k-tiles before they are committed to LDS (one k-tile
    // of MFMAs is ~0.5 us; an L2/MALL round trip under load is longer than that).
    f32x4 ra[2][A_PASSES][AV];
    f32x4 rb[2][B_VECS];
    constexpr bool HAD = a_has_had<A>::value;
    f32x4 rh[2][HAD ? A_PASSES : 1];   // second factor of a Hadamard A operand (ADenseHad)
    auto prefetch_a = [&](auto set, int kt) {
        constexpr int S = decltype(set)::value;
#pragma unroll
        for (int p = 0; p < A_PASSES; ++p)
            if (A_ELEMS % NT == 0 || tid + p * NT < A_ELEMS) {
                A::load(rows[p], kt, a_q, ra[S][p]);
                if constexpr (HAD) rh[S][p] = A::load_had(rows[p], kt, a_q);
            }
    };
    auto prefetch_b = [&](auto set, int kt) {
        constexpr int S = decltype(set)::value;
#pragma unroll
        for (int v = 0; v < B_VECS; ++v) {
            const int e = tid + v * NT;
            if (B_ELEMS % NT != 0 && e >= B_ELEMS) continue;
            if constexpr (!P::B_TR) {
                const int kr = e / (BN / 4), n4 = e % (BN / 4);
                rb[S][v] = *reinterpret_cast<const f32x4*>(w + (size_t)(kt * BK + kr) * P::N(args) + n0 + n4 * 4);
            } else {
                // k-tile kt = (tap, c0); element (k'=c0+kq*4.., n') = w[(tap*NP + n0+n')*KP + c0 + kq*4]
                const int TPT = P::KP(args) / BK;
                const int tap = kt / TPT, c0 = (kt % TPT) * BK;
                const int kq = e % 8, np = e / 8;
                size_t wrow;
                if constexpr (has_b_row<P>::value) wrow = (size_t)P::b_row(y, tap, n0 + np);
                else wrow = (size_t)P::tap_index(y, tap) * P::N(args) + n0 + np;
                rb[S][v] = *reinterpret_cast<const f32x4*>(w + wrow * P::KP(args) + c0 + kq * 4);
            }
        }
    };
    auto commit_a = [&](auto set, int stage) {
        constexpr int S = decltype(set)::value;
        float* As = smem + stage * STAGE;
#pragma unroll
        for (int p = 0; p < A_PASSES; ++p) {
            if (A_ELEMS % NT != 0 && tid + p * NT >= A_ELEMS) continue;
#pragma unroll
            for (int j = 0; j < AV; ++j) {
                f32x4 v = ra[S][p][j];
                if constexpr (HAD) v *= rh[S][p];
                *reinterpret_cast<f32x4*>(&As[(p * (NT / APR) + a_r) * LDA + a_q * A::VEC + j * 4]) = v;
            }
        }
    };
    auto commit_b = [&](auto set, int stage) {
        constexpr int S = decltype(set)::value;
        float* Bs = smem + stage * STAGE + BM * LDA;
#pragma unroll
        for (int v = 0; v < B_VECS; ++v) {
            const int e = tid + v * NT;
            if (B_ELEMS % NT != 0 && e >= B_ELEMS) continue;
            if constexpr (!P::B_TR) {
                const int kr = e / (BN / 4), n4 = e % (BN / 4);
                *reinterpret_cast<f32x4*>(&Bs[kr * LDB + n4 * 4]) = rb[S][v];
            } else {
                const int kq = e % 8, np = e / 8;
                *reinterpret_cast<f32x4*>(&Bs[np * LDA + kq * 4]) = rb[S][v];   // [n'][k'] like the A tile
            }
        }
    };
    using Set0 = std::integral_constant<int, 0>;
    using Set1 = std::integral_constant<int, 1>;

    f32x16 acc[P::TM][P::TN];
#pragma unroll
    for (int tm = 0; tm < P::TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < P::TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    // Software pipeline, branch-free body (tile indices are clamped, so the tail re-stages the last
    // tile into the idle stage: harmless).  While stage `cur` (tile it) feeds the matrix pipe, register
    // set (it+1)&1 holds tile it+1 and the other set tile it+2.
    if (my_n > 0) {
        prefetch_a(Set0{}, tile(0)); prefetch_b(Set0{}, tile(0));
        prefetch_a(Set1{}, tile(1)); prefetch_b(Set1{}, tile(1));
        commit_a(Set0{}, 0); commit_b(Set0{}, 0);
        prefetch_a(Set0{}, tile(2)); prefetch_b(Set0{}, tile(2));
    }

    // Epilogue operands (row map, bias / ReLU mask) are fetched here, so the k loop hides their latency and
    // the 16 stores per tile go out back to back.  (vmcnt counts stores as well as loads on gfx9: a
    // load -> wait -> store sequence per element would serialise 16 memory round trips per wave.)
    const int j = lane & 31, h = lane >> 5;
    typename P::Epi epi = P::epi(args, z, y);   // output / bias / mask pointers, pinned in SGPRs for the epilogue
    int mrow[P::TM][16];
    unsigned okmask[P::TM];
    float aux[P::TM][P::TN][16];
#pragma unroll
    for (int tm = 0; tm < P::TM; ++tm) {
        okmask[tm] = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int mv = m0 + (wm * P::TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (vrow_of<P>(args, y, mv, mrow[tm][r])) okmask[tm] |= 1u << r;
            else mrow[tm][r] = 0;
#pragma unroll
            for (int tn = 0; tn < P::TN; ++tn)
                aux[tm][tn][r] = (ABL & 4) ? 1.f : P::epi_load(epi, mrow[tm][r], n0 + (wn * P::TN + tn) * 32 + j);
        }
    }
    __syncthreads();
    int cur = 0;
    auto step = [&](auto set, int it, auto every) {   // set = (it+1)&1: holds tile it+1; refilled with tile it+3.  every: a step that both teams take
        if (TEAMS == 1 || decltype(every)::value || it < my_n) {    // team-uniform; one team: my_n == iters, and a branch here costs the compiler its knowledge of which loads are outstanding
            const float* As = smem + cur * STAGE;
            const int k3 = tile(it + 3);
            mfma_ktile<P::TM, P::TN, LDB, P::B_TR>(As, As + BM * LDA, wm * P::TM * 32, wn * P::TN * 32, lane, acc, [&](int u) {
                if (u == 0) { commit_a(set, cur ^ 1); commit_b(set, cur ^ 1); }   // tile it+1 -> idle stage
                else if (u == 1) prefetch_a(set, k3);                             // tile it+3 global loads
                else if (u == 2) prefetch_b(set, k3);
            });
        }
        __syncthreads();
        cur ^= 1;
    };
    // (pairs, then the odd tail: a conditional second step inside the loop gives the compiler a path "first step, straight back to the
    //  header" on which the set the header consumes is the most recently loaded one, and its s_waitcnt insertion then drains the loads of
    //  the previous step at every header - seen as vmcnt(3 .. 0) instead of vmcnt(7 .. 4) in the l1 forward kernel)
    if constexpr (TEAMS == 2 && PEEL) {
        // Two teams: the team-uniform `it < my_n` in front of every step is such a path too - a step that is skipped loads nothing - and
        // conv3's dX waited vmcnt(3 .. 0) at every header: its global loads ran one k-tile ahead of their commit, not two.  Team 1 is
        // short by at most one tile, so every step but the last runs without the test (vmcnt(7 .. 4) in the loop).
        const int common = max(iters - 1, 0);
        int it = 0;
        for (; it + 1 < common; it += 2) {
            step(Set1{}, it, std::true_type{});
            step(Set0{}, it + 1, std::true_type{});
        }
        if (it < common) {
            step(Set1{}, it, std::true_type{});
            step(Set0{}, it + 1, std::false_type{});
        } else if (iters > 0) step(Set1{}, it, std::false_type{});
    } else {
        int it = 0;
        for (; it + 1 < iters; it += 2) {
            step(Set1{}, it, std::false_type{});
            step(Set0{}, it + 1, std::false_type{});
        }
        if (it < iters) step(Set1{}, it, std::false_type{});
    }
    if constexpr (TEAMS == 2) {   // acc(team 0) += acc(team 1), through team 1's (now idle) stages
        constexpr int PER_WAVE = P::TM * P::TN * 16 * 64;
        static_assert(2 * STAGE >= NW * PER_WAVE, "team reduction buffer");
        float* red = smem_all + 2 * STAGE;
        if (team == 1) {
#pragma unroll
            for (int tm = 0; tm < P::TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < P::TN; ++tn)
#pragma unroll
                    for (int r = 0; r < 16; ++r) red[wave * PER_WAVE + ((tm * P::TN + tn) * 16 + r) * 64 + lane] = acc[tm][tn][r];
        }
        __syncthreads();
        if (team == 1) return;
#pragma unroll
        for (int tm = 0; tm < P::TM; ++tm)
#pragma unroll
            for (int tn = 0; tn < P::TN; ++tn)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[tm][tn][r] += red[wave * PER_WAVE + ((tm * P::TN + tn) * 16 + r) * 64 + lane];
    }

#pragma unroll
    for (int tm = 0; tm < P::TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < P::TN; ++tn) {
            const int n = n0 + (wn * P::TN + tn) * 32 + j;
            // land the operand loads here, in straight-line code: otherwise every conditional store block
            // gets its own vmcnt(0), which also waits for the previous block's store
#pragma unroll
            for (int r = 0; r < 16; ++r) asm volatile("" ::"v"(aux[tm][tn][r]));
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if ((okmask[tm] >> r & 1) && !((ABL & 2) && acc[tm][tn][r] != 12345.f)) P::store(epi, mrow[tm][r], n, acc[tm][tn][r], aux[tm][tn][r]);
        }
