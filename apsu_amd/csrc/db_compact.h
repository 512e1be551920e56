// Which BinBundles of one bundle index are merged (Engine::compact, apsu_he_db_compact), as a pure function of their bin counts.  No
// HIP in here; the CPU tier reaches it through the emulation library (emu/db.cpp: emu_plan_compaction,
// tests/test_bundle_merge_cpu.py).
//
// The placement rule (db_place.h) tries BinBundles newest first and drops one only when it is empty, so after insertions and removals
// a bundle index keeps several half-empty BinBundles, and each of them costs a query its fixed share (the high-power products, a key
// switch, a result ciphertext).  The rule here, deterministic:
//   * walk the BinBundles in cache order;
//   * a BinBundle joins the FIRST earlier group that (a) has the same set of bins -- the same slots hold the zero polynomial,
//     LOOKUP_NONE -- and (b) has room: count_group[s] + count_bundle[s] < max_items_per_bin for every bin s.  The comparison is strict,
//     as in the placement rule, so no merged bin holds more than max_items_per_bin - 1 items;
//   * otherwise it opens a new group;
//   * a group's counts grow as BinBundles join it.
// A group's degree is max_s of its counts (0 for a group without bins).
#pragma once
#include <algorithm>
#include <vector>

#include "bin_lookup.h"

namespace apsu_he {

struct CompactPlan {
    std::vector<u32> group;                               // [n_bundles]: group ids 0, 1, .. in order of first member
    std::vector<u32> degree;                              // [groups]
    std::vector<u32> counts;                              // [groups][n]
};

// counts[n_bundles][n], cache order; LOOKUP_NONE: the slot is not a bin
inline CompactPlan plan_compaction(const u32 *counts, u32 n_bundles, size_t n, u32 max_items)
{
    CompactPlan plan;
    plan.group.assign(n_bundles, 0);
    for (u32 b = 0; b < n_bundles; b++) {
        const u32 *c = counts + (size_t)b * n;
        const size_t groups = plan.degree.size();
        size_t g = 0;
        for (; g < groups; g++) {
            const u32 *gc = plan.counts.data() + g * n;
            bool fits = true;
            for (size_t s = 0; s < n && fits; s++)
                fits = c[s] == LOOKUP_NONE ? gc[s] == LOOKUP_NONE : gc[s] != LOOKUP_NONE && (u64)gc[s] + c[s] < max_items;
            if (fits) break;
        }
        if (g == groups) {
            plan.counts.insert(plan.counts.end(), c, c + n);
            plan.degree.push_back(0);
        } else {
            u32 *gc = plan.counts.data() + g * n;
            for (size_t s = 0; s < n; s++)
                if (c[s] != LOOKUP_NONE) gc[s] += c[s];
        }
        plan.group[b] = (u32)g;
    }
    for (size_t g = 0; g < plan.degree.size(); g++)
        for (size_t s = 0; s < n; s++)
            if (plan.counts[g * n + s] != LOOKUP_NONE) plan.degree[g] = std::max(plan.degree[g], plan.counts[g * n + s]);
    return plan;
}

}  // namespace apsu_he
