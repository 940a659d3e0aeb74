// ================================================================================================
// Group acting (group_act.hpp), the part without HIP in it: which members a call selects, where every selected member's rows and
// results stand in the two staging areas, the cap of one call, and the draws of the noise stream each member takes.  The acting call
// of a BC group and of an IQL group and tests/test_group_act_plan_host.py (compiled with the host compiler alone) read the rule from
// here.
//   selection   members == nullptr: every member, and n_sel must be P.  A list is strictly ascending, every entry < P, not empty.
//   rows        the selected members' rows stand one behind the other in selection order, every block rounded up to 16 bytes: member
//               b's block starts at row_off[b] and holds n * O elements of 4 (f32) or 8 (float64) bytes.  Two members on one host
//               pointer still get a block each: the kernel reads a member's block only.
//   results     [n_sel][n][A] floats in selection order: member b's block starts at float b * n * A.
//   cap         staged rows and results of one call are at most GA_STAGE_MAX bytes each.
//   draws       a selected member in train mode takes n * A draws at its own noise counter, which then advances by n * A; a member in
//               eval mode, and a member that is not selected, takes none.  A refused plan moves no counter: ga_apply_draws is called
//               only with a plan that ga_plan has accepted.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bdr {

constexpr size_t GA_STAGE_MAX = (size_t)64 << 20;   // staged rows (and results) of one call
constexpr uint64_t GA_MAX_ROWS = 65536;             // rows of one member in one call

enum GaRefusal { GA_OK = 0, GA_EMPTY, GA_RANGE, GA_ORDER, GA_COUNT, GA_ROWS, GA_CAP };

// what ga_select has to say about a member list: `entry` is the offending entry of the list (GA_RANGE, GA_ORDER)
struct GaSelect { int refusal; uint32_t entry; };

inline GaSelect ga_select(const uint32_t* members, uint32_t n_sel, uint32_t P)
{
    if (n_sel < 1) return GaSelect{GA_EMPTY, 0};
    for (uint32_t b = 0; members && b < n_sel; ++b) {
        if (members[b] >= P) return GaSelect{GA_RANGE, b};
        if (b > 0 && members[b] <= members[b - 1]) return GaSelect{GA_ORDER, b};
    }
    if (!members && n_sel != P) return GaSelect{GA_COUNT, 0};
    return GaSelect{GA_OK, 0};
}
inline uint32_t ga_member_at(const uint32_t* members, uint32_t b) { return members ? members[b] : b; }

inline size_t ga_round16(size_t bytes) { return (bytes + 15) / 16 * 16; }
// the bytes of one member's n rows of O elements, f64 or f32
inline size_t ga_row_bytes(int O, bool f64) { return (size_t)O * (f64 ? 8 : 4); }

// the staged layout of one call
struct GaPlan {
    int refusal = GA_OK;
    std::vector<size_t> row_off;   // [n_sel] bytes from the start of the row area, each a multiple of 16
    std::vector<size_t> res_off;   // [n_sel] floats from the start of the result area
    size_t staged = 0;             // bytes of the row area this call fills
    size_t res_floats = 0;         // floats of the result area this call fills
};

// f64[p] (indexed by MEMBER): member p's rows are float64.  Entries of members that are not selected are not read.
inline GaPlan ga_plan(const uint32_t* members, uint32_t n_sel, uint32_t P, uint64_t n, int O, int A, const int* f64)
{
    GaPlan pl;
    const GaSelect s = ga_select(members, n_sel, P);
    if (s.refusal != GA_OK) { pl.refusal = s.refusal; return pl; }
    if (n < 1 || n > GA_MAX_ROWS) { pl.refusal = GA_ROWS; return pl; }
    size_t off = 0;
    for (uint32_t b = 0; b < n_sel; ++b) {
        const uint32_t p = ga_member_at(members, b);
        pl.row_off.push_back(off);
        pl.res_off.push_back((size_t)b * n * A);
        off += ga_round16((size_t)n * ga_row_bytes(O, f64[p] != 0));
    }
    pl.staged = off;
    pl.res_floats = (size_t)n_sel * n * A;
    if (pl.staged > GA_STAGE_MAX || pl.res_floats * 4 > GA_STAGE_MAX) pl.refusal = GA_CAP;
    return pl;
}

// the draws member p takes in a call of n rows: n * A when it is selected and in train mode
inline uint64_t ga_draws(bool selected, bool train, uint64_t n, int A) { return selected && train ? n * (uint64_t)A : 0; }

// the counters of an ACCEPTED call: start[b] = selected member b's counter before the call; counters[p] advances by the member's draws.
// train / counters are indexed by member.  A refused plan changes nothing.
inline void ga_apply_draws(const GaPlan& pl, const uint32_t* members, uint32_t n_sel, uint64_t n, int A, const int* train, uint64_t* counters, uint64_t* start)
{
    if (pl.refusal != GA_OK) return;
    for (uint32_t b = 0; b < n_sel; ++b) {
        const uint32_t p = ga_member_at(members, b);
        if (start) start[b] = counters[p];
        counters[p] += ga_draws(true, train[p] != 0, n, A);
    }
}

}  // namespace bdr
