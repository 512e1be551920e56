// Moving the BinBundles of a resident database to other parameters (Engine::adopt_bundle, rebase), as pure functions.  No HIP in here;
// the CPU tier reaches them through the emulation library (emu/db.cpp: emu_rebase_compatible, emu_rebase_plan,
// tests/test_bundle_split_cpu.py).
//
// Two parameter sets hold the same database in the same bins when the ring, the plain modulus and the table and item geometry agree:
// every item then lies in the same bin of the same bundle index, and a stored plaintext is the same polynomial mod t.  What may differ
// is how that polynomial is stored (the coefficient primes, the Paterson-Stockmeyer slots of ps_low_degree), what a query sends
// (query_powers) and how full a bin may be (max_items_per_bin); only the last can ask for a split.
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "bin_split.h"
#include "params.h"

namespace apsu_he {

// empty: BinBundles of src can be moved to dst; else a sentence naming the first field that differs
inline std::string rebase_compatible(const PSUParams &src, const PSUParams &dst)
{
    auto differs = [](const char *field, u64 a, u64 b) {
        return std::string(field) + " differs: the source has " + std::to_string(a) + ", the destination " + std::to_string(b);
    };
    if (src.seal_params.poly_modulus_degree != dst.seal_params.poly_modulus_degree)
        return differs("poly_modulus_degree", src.seal_params.poly_modulus_degree, dst.seal_params.poly_modulus_degree);
    if (src.seal_params.plain_modulus != dst.seal_params.plain_modulus) return differs("plain_modulus", src.seal_params.plain_modulus, dst.seal_params.plain_modulus);
    if (src.item_params.felts_per_item != dst.item_params.felts_per_item) return differs("felts_per_item", src.item_params.felts_per_item, dst.item_params.felts_per_item);
    if (src.table_params.table_size != dst.table_params.table_size) return differs("table_size", src.table_params.table_size, dst.table_params.table_size);
    if (src.table_params.hash_func_count != dst.table_params.hash_func_count)
        return differs("hash_func_count", src.table_params.hash_func_count, dst.table_params.hash_func_count);
    return std::string();
}

// Per input BinBundle its number of parts (split_parts of its largest bin under the destination's max_items_per_bin) and the cache_idx of
// each part: dense per bundle index, in input order, the parts of one BinBundle consecutive.
struct RebasePlan {
    std::vector<u32> parts;                               // [n_bundles]
    std::vector<u32> first;                               // [n_bundles]: the position of its part 0 in cache_idx / origin
    std::vector<u32> cache_idx, origin;                   // [sum of parts]
};
// max_count[b]: the largest bin count of BinBundle b (0 for one without bins)
inline RebasePlan rebase_plan(const u32 *max_count, const u32 *bundle_idx, u32 n_bundles, u32 dst_max_items)
{
    RebasePlan plan;
    std::vector<std::pair<u32, u32>> next;                // (bundle index, its next cache_idx), few of them
    for (u32 b = 0; b < n_bundles; b++) {
        const u32 k = split_parts(max_count[b], dst_max_items);
        size_t at = 0;
        while (at < next.size() && next[at].first != bundle_idx[b]) at++;
        if (at == next.size()) next.emplace_back(bundle_idx[b], 0);
        plan.parts.push_back(k);
        plan.first.push_back((u32)plan.cache_idx.size());
        for (u32 p = 0; p < k; p++) {
            plan.cache_idx.push_back(next[at].second++);
            plan.origin.push_back(b);
        }
    }
    return plan;
}

}  // namespace apsu_he
