// Building a whole database from its entries (Engine::build_from_entries): the placement rule in closed form, and the lane body of
// k_entries_scatter (kernels_db.hip).  No HIP in here; the CPU tier reaches it through the emulation library (emu_bulk/bulk.cpp:
// emu_bulk_plan, emu_entries_scatter in libapsu_he_hostemu_bulk.so; tests/test_bulk_place_cpu.py).
//
// ReceiverDB::set_data is clear plus insert_or_assign_worker on an empty database (receiver_db.cpp:349-434): the entries of cuckoo
// location 0, 1, .. in list order, each tried on the BinBundles of its bundle index newest first, fitting iff every bin it touches
// holds fewer than max_items_per_bin - 1 items (:388-389, strictly), else a new BinBundle takes it (:410-433).  place_entries
// (db_place.h) restates that loop entry by entry.  On an EMPTY database it has a closed form, because the bins of two locations of one
// bundle index never overlap -- location l owns bins (l % items_per_bundle) F .. + F - 1 -- so a location meets nothing but the NUMBER
// of BinBundles the locations before it have opened:
//   cap = max_items_per_bin - 1 entries of one location fit one BinBundle.
//   K_l = the BinBundles of l's bundle index when l begins = max over the earlier locations l' of that index of ceil(c_l' / cap).
//   Entry i of location l (0-based, list order) is in chunk m = i / cap.  m < K_l: it goes to BinBundle K_l - 1 - m (the existing
//   ones, newest first); else to BinBundle m (opened by this location, in order).  Its position in its bins is i - m cap.
// Nothing is deduplicated (the reference's loop does not: hashed_items_ dedupes ITEMS before the OPRF): two equal entries of one
// location put a double root into their bins.  place_entries calls the second a DUPLICATE, so the two rules agree on lists whose
// entries are distinct per location, which is what the contract is stated for.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "cuckoo.h"

namespace apsu_he {

struct BulkPlan {
    std::vector<u32> kstart;                              // [T]: K_l, restarting at 0 with every bundle index
    std::vector<u32> bundles;                             // [T / items_per_bundle]: BinBundles per bundle index
    u64 total = 0;                                        // their sum
};

// offsets[T + 1]: location l holds entries offsets[l] .. offsets[l + 1] (apsu_he_items_bucket's).  Every refusal: std::invalid_argument
inline BulkPlan bulk_plan(const u64 *offsets, size_t T, u32 items_per_bundle, u32 max_items_per_bin)
{
    if (max_items_per_bin < 2) throw std::invalid_argument("bulk_plan: max_items_per_bin = " + std::to_string(max_items_per_bin) + " leaves no room in a bin (an entry fits below max_items_per_bin - 1 items)");
    if (!items_per_bundle || T % items_per_bundle) throw std::invalid_argument("bulk_plan: " + std::to_string(T) + " locations are not bundle_idx_count * items_per_bundle");
    const u32 cap = max_items_per_bin - 1;
    BulkPlan p;
    p.kstart.assign(T, 0);
    p.bundles.assign(T / items_per_bundle, 0);
    for (size_t l = 0; l < T; l++) {
        if (offsets[l + 1] < offsets[l]) throw std::invalid_argument("bulk_plan: offsets decrease at location " + std::to_string(l));
        const u64 c = offsets[l + 1] - offsets[l];
        if (c > 0xFFFFFFFFull) throw std::invalid_argument("bulk_plan: location " + std::to_string(l) + " holds more than 2^32 - 1 entries");
        u32 &K = p.bundles[l / items_per_bundle];
        p.kstart[l] = K;
        const u32 chunks = (u32)((c + cap - 1) / cap);
        if (chunks > K) K = chunks;
    }
    for (u32 K : p.bundles) p.total += K;
    return p;
}

struct BulkChunk { u32 first, len; };

// the entries first .. first + len - 1 of a location with c entries that BinBundle k takes; len == 0: none
HD BulkChunk bulk_chunk(u32 kstart, u32 c, u32 k, u32 cap)
{
    const u64 m = k < kstart ? (u64)(kstart - 1 - k) : (u64)k;
    const u64 first = m * cap;
    BulkChunk ch;
    ch.first = first < c ? (u32)first : 0;
    ch.len = first < c ? (c - first < cap ? (u32)(c - first) : cap) : 0;
    return ch;
}

// the degree of BinBundle k of a bundle index whose `locations` counts and kstart are given: the largest chunk
inline u32 bulk_degree(const u64 *offsets, const u32 *kstart, u32 locations, u32 k, u32 cap)
{
    u32 degree = 0;
    for (u32 l = 0; l < locations; l++) {
        const u32 len = bulk_chunk(kstart[l], (u32)(offsets[l + 1] - offsets[l]), k, cap).len;
        if (len > degree) degree = len;
    }
    return degree;
}

struct alignas(16) BulkItem { u64 lo, hi; };              // one post-OPRF item: its 128 bits, little-endian (one 16-byte load)

constexpr int SCATTER_T = 256;                            // lanes per workgroup of k_entries_scatter
constexpr u32 SCATTER_MAX_F = 64;                         // felts_per_item the kernel admits (lanes 0 .. F - 1 write a location's counts)

// The body of one lane of k_entries_scatter for target BinBundle k of one bundle index: workgroup (loc, by) of a grid of
// (locations + 1) x gy workgroups of T lanes, lane tid.  items: the bundle index's entries; offsets[locations + 1] and kstart[locations]:
// its slices (items[0] is entry offsets[0]).  Row `loc` < locations: the lane is the entry -- entry r of the location's chunk is one
// 16-byte load and F stores roots[(loc F + j) stride + r], so for fixed j a wave writes consecutive words; the lanes j < F of the row's
// first workgroup write counts[loc F + j] = len.  Row `locations`: its first workgroup zeroes the counts of the slots no location owns,
// locations F .. n_counts - 1.  Words of roots at or beyond a bin's count are not written.
HD void entries_scatter_lane(const BulkItem *items, const u64 *offsets, const u32 *kstart, u32 locations, u32 F, u32 bpf, u32 item_bits, u32 cap,
                             u32 k, u32 stride, u64 *roots, u32 *counts, u32 n_counts, u32 loc, u32 by, u32 gy, u32 tid, u32 T)
{
    if (loc >= locations) {
        if (by == 0)
            for (u32 s = locations * F + tid; s < n_counts; s += T) counts[s] = 0;
        return;
    }
    const u64 o0 = offsets[loc];
    const BulkChunk ch = bulk_chunk(kstart[loc], (u32)(offsets[loc + 1] - o0), k, cap);
    const u32 s = loc * F;
    if (by == 0 && tid < F) counts[s + tid] = ch.len;
    const BulkItem *src = items + (o0 - offsets[0]) + ch.first;
    for (u32 r = by * T + tid; r < ch.len; r += gy * T) {
        const BulkItem it = src[r];
        for (u32 j = 0; j < F; j++) roots[(size_t)(s + j) * stride + r] = cuckoo_item_felt(it.lo, it.hi, j, bpf, item_bits);
    }
}

// workgroups per location: one per SCATTER_T entries of a full chunk (location x block of entries), fewer where that would take the grid
// beyond about 16384 workgroups (the stride loop covers the rest).  Measured at 16M-4096 (1638 locations, cap 1303) with 1, 2 and 6
// per location: 6, this rule's choice, was the fastest (profiles/r27_bulk_build.txt)
inline u32 scatter_blocks(u32 locations, u32 cap)
{
    const u32 per_chunk = (cap + SCATTER_T - 1) / SCATTER_T;
    const u32 most = 16384 / (locations + 1);
    return per_chunk < most ? (per_chunk ? per_chunk : 1) : (most ? most : 1);
}

} // namespace apsu_he
