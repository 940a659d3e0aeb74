// The index arithmetic of the grouped prioritized-replay kernels (border_amd/csrc/per.hip k_per_*_group) on the CPU: the functions of
// csrc/per_tree.hpp over bounds-checked host arrays, on the schedules the kernels use - one "workgroup" per member with its phases
// separated where the kernel has a barrier, the (depth, entry) pairs of the update's fold, the one-lane-per-ancestor walk of a
// single-row push, the staged top of the tree and the three-level fetch of the descent.  Stand-alone: build with
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/group_per_sim.cpp -o group_per_sim
// and run it directly (tests/test_group_per_host.py does).
//
//   group_per_sim CAPACITY NORMALIZE(0 All | 1 Batch) ALPHA SCRIPT
// SCRIPT holds one operation per line (floats as the hex of their bits):
//   P                        push one row at the head (set_priority(1): the current maximum priority)
//   S n beta u_0 .. u_n-1    sample n <= 128 rows with these uniforms         -> "S ix_0 .. ix_n-1 | w_0 .. w_n-1"
//   U n ix_0 td_0 ..         update_priority of n <= 128 (index, |td|) pairs
//   T                        print the tree                                   -> "T node_0 .. node_len-1"
// pow is the host's f64 pow, as powf_ref is the device's: alpha = 1 makes every priority exact.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../border_amd/csrc/per_tree.hpp"

using namespace bdr;

namespace {

[[noreturn]] void die(const char* what, uint64_t i, uint64_t n)
{
    fprintf(stderr, "out of bounds: %s[%llu] of %llu\n", what, (unsigned long long)i, (unsigned long long)n);
    exit(3);
}

template <class T>
struct Checked {   // every access is checked: an index the kernels would send out of an array ends the program
    std::vector<T> v; const char* name;
    Checked(const char* nm, size_t n, T fill) : v(n, fill), name(nm) {}
    T& operator[](uint64_t i) { if (i >= v.size()) die(name, i, v.size()); return v[i]; }
};

constexpr int GROUP_B = 128, PAD = GROUP_B + 8, WG = 256;
constexpr float MM_MIN_INIT = FLT_MAX, MM_MAX_INIT = 1e-8f;

float powf_ref(float x, float y) { return (float)pow((double)x, (double)y); }
float from_bits(const std::string& s) { const uint32_t b = (uint32_t)strtoul(s.c_str(), nullptr, 16); float f; memcpy(&f, &b, 4); return f; }
unsigned bits(float f) { unsigned b; memcpy(&b, &f, 4); return b; }

struct Member {
    uint64_t capacity, len, head = 0, n_samples = 0;
    int normalize, maxdepth;
    float alpha, eps = 1e-8f;
    Checked<float> tree;
    float mm[2] = {MM_MIN_INIT, MM_MAX_INIT};
    bool mm_valid = false;
    Member(uint64_t c, int nz, float a) : capacity(c), len(per_tree_len(c)), normalize(nz), maxdepth(per_max_depth(c)), alpha(a), tree("tree", 2 * c - 1, 0.f) {}

    // k_per_minmax_group: blocks of 2048 leaves, i < capacity
    void minmax()
    {
        for (uint64_t block = 0; block * 2048 < capacity; ++block)
            for (int t = 0; t < WG; ++t)
                for (int u = 0; u < 8; ++u) {
                    const uint64_t i = block * 2048 + (uint64_t)t + (uint64_t)u * 256;
                    const float v = i < capacity ? tree[capacity - 1 + i] : 0.f;
                    mm[1] = fmaxf(mm[1], v);
                    if (i < n_samples) mm[0] = fminf(mm[0], v);
                }
    }
    void take(float& mn, float& mx) { mn = mm[0]; mx = mm[1]; mm[0] = MM_MIN_INIT; mm[1] = MM_MAX_INIT; }

    // k_per_push_group: one wave, lane d takes the ancestor at depth d
    void push()
    {
        if (!mm_valid) minmax();
        float mn, mx;
        take(mn, mx);
        mm_valid = false;
        if (head >= capacity) die("head", head, capacity);
        const uint64_t leaf = head + capacity - 1;
        const float old = tree[leaf];
        const float praw = powf_ref(mx, 1.0f / alpha);
        const float p = powf_ref(praw + eps, alpha);
        bool bad;
        const float change = per_change(p, old, bad);
        const int dl = per_node_depth(leaf);
        if (dl > 63) die("lanes", (uint64_t)dl, 64);
        for (int lane = 0; lane < 64; ++lane)
            if (lane < dl) { const uint64_t nd = per_ancestor(leaf, dl, lane); tree[nd] = tree[nd] + change; }
        if (!bad) tree[leaf] = p;
        head = (head + 1) % capacity;
        n_samples = n_samples + 1 < capacity ? n_samples + 1 : capacity;
    }

    // k_per_sample_group
    void sample(int n, float beta, const std::vector<float>& us)
    {
        if (n > GROUP_B) die("batch", (uint64_t)n, GROUP_B);
        float mn = FLT_MAX, mx;
        if (normalize == 0) { if (!mm_valid) minmax(); take(mn, mx); }
        mm_valid = false;
        Checked<float> s_top("s_top", PER_TOP_NODES, 0.f);
        const uint64_t ntop = per_top_nodes(len);
        for (int t = 0; t < WG; ++t) for (uint64_t i = (uint64_t)t; i < ntop; i += WG) s_top[i] = tree[i];
        const float p_sum = s_top[0];
        const float nn = (float)n_samples / p_sum;
        std::vector<uint64_t> ixs(n);
        std::vector<float> wk(WG, -FLT_MAX);
        for (int k = 0; k < n; ++k) {
            const float s = p_sum * us[k];
            const uint64_t node = per_descend(s, len, ntop, [&](uint64_t i) { return s_top[i]; }, [&](uint64_t i) { return tree[i]; });
            if (node + 1 < capacity || node >= len) die("leaf", node, len);
            ixs[k] = node + 1 - capacity;
            wk[k] = powf_ref(nn * tree[node], -beta);
        }
        float w_max_inv;
        if (normalize == 0) w_max_inv = powf_ref(nn * mn, beta);
        else {
            float m = -FLT_MAX;
            for (int k = 0; k < WG; ++k) m = fmaxf(m, wk[k]);
            w_max_inv = 1.0f / m;
        }
        printf("S");
        for (int k = 0; k < n; ++k) printf(" %llu", (unsigned long long)ixs[k]);
        printf(" |");
        for (int k = 0; k < n; ++k) printf(" %08x", bits(wk[k] * w_max_inv));
        printf("\n");
    }

    // k_per_update_group
    void update(int n, const std::vector<uint64_t>& ixs, const std::vector<float>& td)
    {
        if (n > GROUP_B) die("batch", (uint64_t)n, GROUP_B);
        Checked<uint32_t> s_ix("s_ix", PAD, PER_NO_NODE), s_leaf("s_leaf", PAD, 0u);
        Checked<int> s_dl("s_dl", PAD, 0);
        Checked<float> s_p("s_p", GROUP_B, 0.f), s_change("s_change", PAD, 0.f);
        mm[0] = MM_MIN_INIT; mm[1] = MM_MAX_INIT;
        std::vector<char> live(WG, 0), last(WG, 0);
        std::vector<float> old(WG, 0.f);
        for (int t = 0; t < WG; ++t) if (t < n) {
            live[t] = ixs[t] < capacity;
            s_ix[t] = live[t] ? (uint32_t)ixs[t] : PER_NO_NODE;
            s_p[t] = powf_ref(td[t] + eps, alpha);
        }
        for (int t = 0; t < WG; ++t) if (live[t]) {
            int prev; bool lst;
            per_dup_scan([&](int j) { return s_ix[j]; }, n, t, s_ix[t], prev, lst);
            last[t] = lst;
            old[t] = prev >= 0 ? s_p[prev] : tree[(uint64_t)s_ix[t] + capacity - 1];
        }
        for (int t = 0; t < WG; ++t) if (live[t]) {
            bool bad;
            const float change = per_change(s_p[t], old[t], bad);
            const uint64_t leaf = (uint64_t)s_ix[t] + capacity - 1;
            s_change[t] = change; s_leaf[t] = (uint32_t)leaf; s_dl[t] = per_node_depth(leaf);
            if (last[t] && !bad) tree[leaf] = s_p[t];
        }
        const int total = maxdepth * n;
        for (int t = 0; t < WG; ++t)
            for (int e = t; e < total; e += WG) {
                const int d = e / n, k = e % n;
                auto node = [&](int j) { return per_ancestor_or_none(s_leaf[j], s_dl[j], d); };
                const uint32_t nd = node(k);
                if (nd == PER_NO_NODE) continue;
                if (!per_fold_owner(node, k, nd)) continue;
                tree[nd] = per_fold(tree[nd], node, [&](int j) { return s_change[j]; }, k, n, nd);
            }
        if (normalize == 0) { minmax(); mm_valid = true; } else mm_valid = false;
    }
};

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 5) { fprintf(stderr, "usage: group_per_sim CAPACITY NORMALIZE ALPHA SCRIPT\n"); return 2; }
    const uint64_t capacity = strtoull(argv[1], nullptr, 10);
    if (capacity < 2 || capacity >= (1ull << 31)) { fprintf(stderr, "2 <= capacity < 2^31\n"); return 2; }
    Member m(capacity, atoi(argv[2]), strtof(argv[3], nullptr));
    std::ifstream in(argv[4]);
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[4]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string op, tok;
        if (!(ls >> op)) continue;
        if (op == "P") m.push();
        else if (op == "T") {
            printf("T");
            for (uint64_t i = 0; i < m.len; ++i) printf(" %08x", bits(m.tree[i]));
            printf("\n");
        } else if (op == "S") {
            int n; ls >> n >> tok;
            const float beta = from_bits(tok);
            std::vector<float> us;
            while (ls >> tok) us.push_back(from_bits(tok));
            if ((int)us.size() != n) { fprintf(stderr, "S: %d uniforms expected\n", n); return 2; }
            m.sample(n, beta, us);
        } else if (op == "U") {
            int n; ls >> n;
            std::vector<uint64_t> ixs; std::vector<float> td;
            for (int k = 0; k < n; ++k) { uint64_t ix; ls >> ix >> tok; ixs.push_back(ix); td.push_back(from_bits(tok)); }
            if (!ls) { fprintf(stderr, "U: %d pairs expected\n", n); return 2; }
            m.update(n, ixs, td);
        } else { fprintf(stderr, "unknown operation %s\n", op.c_str()); return 2; }
    }
    return 0;
}
