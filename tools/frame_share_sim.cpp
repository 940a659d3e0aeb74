// The sharing rule of the single-frame store (border_amd/csrc/frame_share.hpp) on its own, without a GPU: reads stacked rows from a
// file, answers the rule's equality questions with memcmp - as the host push does - and prints what every transition was given.
// tests/test_frame_share_host.py builds it with -fsanitize=address,undefined and compares the output with its own restatement.
//
//   frame_share_sim K FRAME_BYTES CAPACITY FRAME_CAPACITY N FILE      FILE: N x (obs row | next_obs row), rows of K * FRAME_BYTES
// per transition:  "s oseq.. | nseq.. | first_ref | src:frame:seq .."      (sequence numbers newest frame first)
// a transition the store cannot hold: "s exhausted" and the program ends (exit status 0: the rule said so, nothing went wrong)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../border_amd/csrc/frame_share.hpp"

int main(int argc, char** argv)
{
    if (argc != 7) { fprintf(stderr, "usage: %s K FRAME_BYTES CAPACITY FRAME_CAPACITY N FILE\n", argv[0]); return 2; }
    const int k = atoi(argv[1]);
    const uint64_t fb = strtoull(argv[2], nullptr, 10), capacity = strtoull(argv[3], nullptr, 10), frame_cap = strtoull(argv[4], nullptr, 10),
                   n = strtoull(argv[5], nullptr, 10);
    if (k < 1 || fb == 0 || capacity == 0 || frame_cap < (uint64_t)2 * k + 1) { fprintf(stderr, "bad arguments\n"); return 2; }
    const uint64_t row = (uint64_t)k * fb;
    std::vector<uint8_t> rows(n * 2 * row), last_next(row);
    FILE* fp = fopen(argv[6], "rb");
    if (!fp || fread(rows.data(), 1, rows.size(), fp) != rows.size()) { fprintf(stderr, "cannot read %llu bytes from %s\n", (unsigned long long)rows.size(), argv[6]); return 2; }
    fclose(fp);
    bdr::FrameShare f;
    f.init(k, capacity, frame_cap);
    uint64_t i = 0, size = 0;
    for (uint64_t s = 0; s < n; ++s) {
        const uint8_t* os = rows.data() + s * 2 * row;
        const uint8_t* ns = os + row;
        auto eq = [&](int q) -> bool {
            const uint8_t *u, *v;
            if (q < k) { u = os + (uint64_t)q * fb; v = last_next.data() + (uint64_t)q * fb; }
            else if (q < 2 * k - 1) { const uint64_t j = q - k; u = os + j * fb; v = os + (j + 1) * fb; }
            else if (q < 3 * k - 2) { const uint64_t j = q - (2 * k - 1); u = ns + (j + 1) * fb; v = os + j * fb; }
            else { const uint64_t j = q - (3 * k - 2); u = ns + j * fb; v = ns + (j + 1) * fb; }
            return memcmp(u, v, fb) == 0;
        };
        std::string allocs;
        auto on_alloc = [&](int src, int j, uint64_t seq) { allocs += " " + std::string(src ? "n" : "o") + ":" + std::to_string(j) + ":" + std::to_string(seq); };
        if (!bdr::frame_share_step(f, i, size, eq, on_alloc)) { printf("%llu exhausted\n", (unsigned long long)s); return 0; }
        printf("%llu", (unsigned long long)s);
        for (int j = 0; j < k; ++j) printf(" %llu", (unsigned long long)f.oseq[j]);
        printf(" |");
        for (int j = 0; j < k; ++j) printf(" %llu", (unsigned long long)f.nseq[j]);
        printf(" | %llu |%s\n", (unsigned long long)f.first_ref[i], allocs.c_str());
        memcpy(last_next.data(), ns, row);
        i = (i + 1) % capacity; size += 1;
    }
    return 0;
}
