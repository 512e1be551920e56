// The rules of a resident database behind the multi-device handle (MultiEngine, multi.h), as pure functions: where a new BinBundle
// goes, what every BinBundle's id is after BinBundles were dropped, replaced, merged or appended, and on which device a merge is made.
// No HIP in here; the CPU tier reaches it through the emulation library (emu/db.cpp: emu_place_new_unit, emu_registry_after,
// emu_index_in_cache_order, emu_merge_home; tests/test_multi_place_cpu.py).  MultiEngine reads these and spells the rules nowhere else.
//
//   * place_new_unit: the candidates of a bundle index are the devices partition_units' first pass gives it (sharding.cpp, devs_of):
//     with at least as many devices as bundle indices the slots r with r % bundle_idx_count == bundle_idx, else the one slot
//     bundle_idx % world.  The candidate with the smallest load takes the BinBundle, ties go to the lowest slot.  load[r] is the sum
//     of unit_cost(degree) = degree + 64 over the BinBundles of device r, partition_units' unit.  Fed a set's units one by one, bundle
//     index by bundle index, in partition_units' order (degree descending, then cache_idx ascending), the rule gives
//     partition_units(set, cost 0) exactly.  The spill pass of partition_units is NOT re-run incrementally: it moves BinBundles that
//     are placed already, which an insertion must not do behind a caller's back (apsu_he_multi_db_move_bundle is the caller's tool).
//   * registry_after: ids stay dense.  Survivors keep their relative order and take 0, 1, ..; appended BinBundles follow in order of
//     appending.  A replaced BinBundle keeps its place (and its slot) with a new degree.  A merge is stated with these two words: the
//     group's first member in cache order is REPLACED by the merged BinBundle, the other members are DROPPED -- so the merged BinBundle
//     takes the place of its group's first member in cache order (the reference renumbers by position too, receiver_db.cpp:551-555).
//   * merge_home: the merged BinBundle is made on the device of the group's first member in cache order; the other members travel.
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace apsu_he {

constexpr uint64_t UNIT_OVERHEAD = 64;                            // relinearisation, epilogue (partition_units)
inline uint64_t unit_cost(uint32_t degree) { return (uint64_t)degree + UNIT_OVERHEAD; }

struct RegUnit {                                                  // one registered BinBundle
    int slot = 0;
    uint32_t bundle_idx = 0, cache_idx = 0, degree = 0;
};

inline bool unit_candidate(int slot, uint32_t bundle_idx, uint32_t bundle_idx_count, int world)
{
    if ((uint32_t)world >= bundle_idx_count) return (uint32_t)slot % bundle_idx_count == bundle_idx;
    return slot == (int)(bundle_idx % (uint32_t)world);
}

inline int place_new_unit(uint32_t bundle_idx, uint32_t bundle_idx_count, int world, const uint64_t *load)
{
    if (world <= 0) throw std::invalid_argument("no devices");
    if (!bundle_idx_count) throw std::invalid_argument("bundle_idx_count is zero");
    if (bundle_idx >= bundle_idx_count) throw std::invalid_argument("bundle_idx out of range");
    int best = -1;
    for (int r = 0; r < world; r++)
        if (unit_candidate(r, bundle_idx, bundle_idx_count, world) && (best < 0 || load[r] < load[best])) best = r;   // ties keep the lowest slot
    return best;
}

inline std::vector<uint64_t> device_loads(const std::vector<RegUnit> &reg, int world)
{
    std::vector<uint64_t> load((size_t)std::max(world, 0), 0);
    for (const RegUnit &u : reg) {
        if (u.slot < 0 || u.slot >= world) throw std::invalid_argument("device slot out of range");
        load[(size_t)u.slot] += unit_cost(u.degree);
    }
    return load;
}

// the ids of one bundle index in cache order (ascending cache_idx); two BinBundles of the index with one cache_idx: std::invalid_argument
inline std::vector<int> index_in_cache_order(const std::vector<RegUnit> &reg, uint32_t bundle_idx)
{
    std::vector<int> ids;
    for (size_t i = 0; i < reg.size(); i++)
        if (reg[i].bundle_idx == bundle_idx) ids.push_back((int)i);
    std::stable_sort(ids.begin(), ids.end(), [&](int a, int b) { return reg[(size_t)a].cache_idx < reg[(size_t)b].cache_idx; });
    for (size_t k = 1; k < ids.size(); k++)
        if (reg[(size_t)ids[k]].cache_idx == reg[(size_t)ids[k - 1]].cache_idx)
            throw std::invalid_argument("BinBundles " + std::to_string(ids[k - 1]) + " and " + std::to_string(ids[k]) + " of bundle index " +
                                        std::to_string(bundle_idx) + " share cache_idx " + std::to_string(reg[(size_t)ids[k]].cache_idx));
    return ids;
}

// the group's first member in cache order: its position among `members` (ties: the earliest given)
inline size_t merge_first(const std::vector<RegUnit> &members)
{
    if (members.empty()) throw std::invalid_argument("a merge group has no members");
    size_t first = 0;
    for (size_t i = 1; i < members.size(); i++)
        if (members[i].cache_idx < members[first].cache_idx) first = i;
    return first;
}
inline int merge_home(const std::vector<RegUnit> &members) { return members[merge_first(members)].slot; }

struct RegistryAfter {
    std::vector<int> new_id;                                      // [old count + appended]: -1 for a dropped id
    std::vector<RegUnit> registry;
};

// dropped[old count]: non-zero = the id leaves.  replaced_degree[old count]: < 0 = unchanged, else the new degree of the BinBundle that
// takes this id's place.  An id cannot be both.  appended: the new BinBundles with their slots, in order of appending.
inline RegistryAfter registry_after(const std::vector<RegUnit> &old, const std::vector<unsigned char> &dropped,
                                    const std::vector<int64_t> &replaced_degree, const std::vector<RegUnit> &appended)
{
    if (dropped.size() != old.size() || replaced_degree.size() != old.size()) throw std::invalid_argument("one entry per registered BinBundle");
    RegistryAfter out;
    out.new_id.assign(old.size() + appended.size(), -1);
    for (size_t i = 0; i < old.size(); i++) {
        if (dropped[i]) {
            if (replaced_degree[i] >= 0) throw std::invalid_argument("BinBundle " + std::to_string(i) + " is both dropped and replaced");
            continue;
        }
        RegUnit u = old[i];
        if (replaced_degree[i] >= 0) u.degree = (uint32_t)replaced_degree[i];
        out.new_id[i] = (int)out.registry.size();
        out.registry.push_back(u);
    }
    for (size_t k = 0; k < appended.size(); k++) {
        out.new_id[old.size() + k] = (int)out.registry.size();
        out.registry.push_back(appended[k]);
    }
    return out;
}

}  // namespace apsu_he
