// The index rules of the prioritized-replay sum tree (sum_tree.rs) as code of their own: the descent of SumTree::sample with its
// multi-level fetch bounds, the ancestor-at-depth formula, the duplicate scan of one update batch with its NaN rule, and the
// in-batch-order fold of one node.  Shared by the kernels of per.hip (k_per_* for one ring, k_per_*_group for the prioritized members
// of an agent group) and by tools/group_per_sim.cpp, which runs them on the CPU over bounds-checked arrays.  Nothing here touches
// memory except through the accessors it is given; powf_ref (the f64 pow) stays with the kernels.
//
// Layout: 2 * capacity - 1 nodes, leaves at capacity - 1 + ix, parent (i - 1) / 2, for ANY capacity >= 2 (leaves may sit at two depths).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PER_HD __host__ __device__ __forceinline__
#define PER_UNROLL _Pragma("unroll")
#else
#define PER_HD inline
#define PER_UNROLL
#endif

namespace bdr {

constexpr int PER_TOP = 13;                                        // the levels a sampling workgroup stages in LDS
constexpr uint32_t PER_TOP_NODES = (1u << PER_TOP) - 1;            // nodes 0 .. 2^13 - 2 (32 KB)
constexpr uint32_t PER_NO_NODE = 0xffffffffu;                      // node ids are < 2 * capacity < 2^32

PER_HD uint64_t per_tree_len(uint64_t capacity) { return 2 * capacity - 1; }
PER_HD uint64_t per_top_nodes(uint64_t len) { return len < (uint64_t)PER_TOP_NODES ? len : (uint64_t)PER_TOP_NODES; }
PER_HD int per_node_depth(uint64_t i) { return 63 - __builtin_clzll((unsigned long long)(i + 1)); }
PER_HD int per_max_depth(uint64_t capacity) { return per_node_depth(2 * capacity - 2); }   // depth of the last leaf
// the ancestor at depth d of the node `leaf` whose own depth is dl (d <= dl)
PER_HD uint64_t per_ancestor(uint64_t leaf, int dl, int d) { return ((leaf + 1) >> (dl - d)) - 1; }
// ... as a 32-bit id, PER_NO_NODE for d >= dl (the leaf itself is assigned, not accumulated)
PER_HD uint32_t per_ancestor_or_none(uint64_t leaf, int dl, int d) { return d < dl ? (uint32_t)per_ancestor(leaf, dl, d) : PER_NO_NODE; }

// retrieve (sum_tree.rs:54-66): `s <= tree[left] || tree[right] == 0` -> left, else s -= tree[left], right
PER_HD void per_descend_step(float& s, uint64_t& ix, float tl, float tr)
{
    if (s <= tl || tr == 0.f) ix = 2 * ix + 1;
    else { s -= tl; ix = 2 * ix + 2; }
}

// The whole descent from the root: returns the NODE of the leaf reached (data index = node + 1 - capacity).
//   top(i)   node i < ntop (ntop = per_top_nodes(len): the staged top of the tree)
//   tree(i)  node i < len
// Below the staged part every round trip fetches the 2 children, 4 grandchildren and 8 great-grandchildren of ix - three contiguous
// runs of the heap - and resolves up to three levels; a run is fetched only when ALL of it exists (g0 + 3 < len, h0 + 7 < len).
template <class Top, class Tree>
PER_HD uint64_t per_descend(float s, uint64_t len, uint64_t ntop, Top top, Tree tree)
{
    uint64_t ix = 0;
    while (2 * ix + 2 < ntop) per_descend_step(s, ix, top(2 * ix + 1), top(2 * ix + 2));   // both children staged
    for (;;) {
        if (2 * ix + 1 >= len) break;                                   // a leaf (an inner node always has both children: len is odd)
        const uint64_t c0 = 2 * ix + 1, g0 = 4 * ix + 3, h0 = 8 * ix + 7;
        const bool lv2 = g0 + 3 < len, lv3 = h0 + 7 < len;
        float c[2], g[4], h[8];
        c[0] = tree(c0); c[1] = tree(c0 + 1);
PER_UNROLL
        for (int q = 0; q < 4; ++q) g[q] = lv2 ? tree(g0 + q) : 0.f;
PER_UNROLL
        for (int q = 0; q < 8; ++q) h[q] = lv3 ? tree(h0 + q) : 0.f;
        const uint64_t base = ix;
        per_descend_step(s, ix, c[0], c[1]);
        if (!lv2) continue;
        const int s1 = (int)(ix - (2 * base + 1));                      // 0 left, 1 right
        per_descend_step(s, ix, g[2 * s1], g[2 * s1 + 1]);
        if (!lv3) continue;
        const int s2 = (int)(ix - (4 * base + 3));                      // 0..3
        per_descend_step(s, ix, h[2 * s2], h[2 * s2 + 1]);
    }
    return ix;
}

// Duplicates of entry k's index among the n entries of one update batch: the latest one before k (-1: none) and whether none follows.
// Break-free, 8 keys per iteration: key(j) must be readable for j < round_up(n, 8) and differ from every real index (PER_NO_NODE)
// for j >= n.
template <class Key>
PER_HD void per_dup_scan(Key key, int n, int k, uint32_t ix, int& prev, bool& last)
{
    prev = -1; last = true;
    for (int j0 = 0; j0 < n; j0 += 8) {
PER_UNROLL
        for (int u = 0; u < 8; ++u) {
            const int j = j0 + u;
            const bool m = key(j) == ix;
            prev = (m && j < k) ? j : prev;
            last = last && !(m && j > k);
        }
    }
}

// change = p - tree[ix] (sum_tree.rs:100); `if change.is_nan() { panic!() }` (:101-104): the update is dropped - change 0, the leaf keeps
// its value - and `bad` tells the caller to raise the flag the host turns into an error
PER_HD float per_change(float p, float old, bool& bad)
{
    const float change = p - old;
    bad = change != change;
    return bad ? 0.f : change;
}

// Entry k's node at one depth is folded by the FIRST entry that touches it: no j < k with the same node.  node(j) readable for
// j < round_up(k, 8).
template <class Node>
PER_HD bool per_fold_owner(Node node, int k, uint32_t nd)
{
    bool first = true;
    for (int j0 = 0; j0 < k; j0 += 8) {
PER_UNROLL
        for (int u = 0; u < 8; ++u) first = first && !(j0 + u < k && node(j0 + u) == nd);
    }
    return first;
}
// tree[parent] += change (sum_tree.rs:48) for every entry j >= k of the same node, in batch order.  node(j), change(j) readable for
// j < k + round_up(n - k, 8), node(j) == PER_NO_NODE for j >= n.
template <class Node, class Change>
PER_HD float per_fold(float v, Node node, Change change, int k, int n, uint32_t nd)
{
    for (int j0 = k; j0 < n; j0 += 8) {
PER_UNROLL
        for (int u = 0; u < 8; ++u) v = node(j0 + u) == nd ? v + change(j0 + u) : v;
    }
    return v;
}

}  // namespace bdr
