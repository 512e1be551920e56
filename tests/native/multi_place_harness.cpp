// Stand-alone driver of apsu_amd/csrc/multi_place.h for AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_multi_place_cpu.py
// compiles and runs it): random registries through registry_after, index_in_cache_order, merge_home and device_loads, place_new_unit
// over every world and index count and against partition_units (sharding.cpp), and every refusal.  Exits 0 and ends its output with "ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <stdexcept>
#include <vector>

#include "multi_place.h"
#include "sharding.h"

using namespace apsu_he;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

template <class F> static bool refuses(F &&fn)
{
    try { fn(); } catch (const std::invalid_argument &) { return true; }
    return false;
}

int main()
{
    std::mt19937_64 rng(0x41505355);
    auto below = [&](uint64_t m) { return (uint64_t)(rng() % m); };

    // ---- place_new_unit: every world and index count, and the LPT property against partition_units without the spill pass
    size_t placed = 0;
    for (int world = 1; world <= 8; world++)
        for (uint32_t count = 1; count <= 5; count++) {
            for (int trial = 0; trial < 20; trial++) {
                std::vector<ShardUnit> units;
                for (uint32_t b = 0; b < count; b++) {
                    const uint32_t k = (uint32_t)below(10);
                    for (uint32_t c = 0; c < k; c++) units.push_back(ShardUnit{ b, c, (uint32_t)(below(4) * 400 + below(2)) });
                }
                std::shuffle(units.begin(), units.end(), rng);
                const std::vector<int> want = partition_units(units, count, world, 0);
                std::vector<uint64_t> load((size_t)world, 0);
                std::vector<int> got(units.size(), -1);
                for (uint32_t b = 0; b < count; b++) {
                    std::vector<size_t> mine;
                    for (size_t i = 0; i < units.size(); i++) if (units[i].bundle_idx == b) mine.push_back(i);
                    std::sort(mine.begin(), mine.end(), [&](size_t x, size_t y) {
                        if (units[x].degree != units[y].degree) return units[x].degree > units[y].degree;
                        return units[x].cache_idx < units[y].cache_idx;
                    });
                    for (size_t i : mine) {
                        got[i] = place_new_unit(b, count, world, load.data());
                        CHECK(got[i] >= 0 && got[i] < world && unit_candidate(got[i], b, count, world));
                        load[(size_t)got[i]] += unit_cost(units[i].degree);
                        placed++;
                    }
                }
                CHECK(got == want);
                std::vector<RegUnit> reg(units.size());
                for (size_t i = 0; i < units.size(); i++) { reg[i].slot = got[i]; reg[i].bundle_idx = units[i].bundle_idx; reg[i].cache_idx = units[i].cache_idx; reg[i].degree = units[i].degree; }
                CHECK(device_loads(reg, world) == load);
            }
        }
    const uint64_t l2[2] = { ~(uint64_t)0, ~(uint64_t)0 - 1 };
    CHECK(place_new_unit(0, 1, 2, l2) == 1);
    CHECK(refuses([&] { place_new_unit(0, 0, 2, l2); }));
    CHECK(refuses([&] { place_new_unit(2, 2, 2, l2); }));
    CHECK(refuses([&] { place_new_unit(0, 1, 0, l2); }));
    CHECK(refuses([&] { std::vector<RegUnit> r(1); r[0].slot = 2; device_loads(r, 2); }));
    CHECK(refuses([&] { std::vector<RegUnit> r(1); r[0].slot = -1; device_loads(r, 2); }));
    CHECK(device_loads({}, 0).empty());

    // ---- registries: cache order, merges stated as replaced + dropped, renumbering
    size_t registries = 0;
    for (int trial = 0; trial < 4000; trial++) {
        const size_t k = (size_t)below(13);
        std::vector<RegUnit> old(k);
        std::vector<uint32_t> cache(40);
        std::iota(cache.begin(), cache.end(), 0u);
        std::shuffle(cache.begin(), cache.end(), rng);
        for (size_t i = 0; i < k; i++) { old[i].slot = (int)below(3); old[i].bundle_idx = (uint32_t)below(2); old[i].cache_idx = cache[i]; old[i].degree = (uint32_t)below(12); }
        std::vector<unsigned char> dropped(k, 0);
        std::vector<int64_t> replaced(k, -1);
        for (uint32_t b = 0; b < 2; b++) {
            const std::vector<int> ids = index_in_cache_order(old, b);
            for (size_t i = 1; i < ids.size(); i++) CHECK(old[(size_t)ids[i - 1]].cache_idx < old[(size_t)ids[i]].cache_idx);
            if (ids.size() >= 2 && below(2)) {                     // merge a random subset of the index
                std::vector<int> g;
                for (int id : ids) if (below(2)) g.push_back(id);
                if (g.size() >= 2) {
                    std::shuffle(g.begin(), g.end(), rng);
                    std::vector<RegUnit> members;
                    for (int id : g) members.push_back(old[(size_t)id]);
                    const size_t first = merge_first(members);
                    CHECK(merge_home(members) == members[first].slot);
                    for (const RegUnit &m : members) CHECK(members[first].cache_idx <= m.cache_idx);
                    for (size_t i = 0; i < g.size(); i++) {
                        if (i == first) replaced[(size_t)g[i]] = (int64_t)below(12);
                        else dropped[(size_t)g[i]] = 1;
                    }
                }
            }
        }
        for (size_t i = 0; i < k; i++) {
            if (dropped[i] || replaced[i] >= 0) continue;
            const uint64_t what = below(4);
            if (what == 0) dropped[i] = 1;
            else if (what == 1) replaced[i] = (int64_t)below(12);
        }
        std::vector<RegUnit> app((size_t)below(4));
        for (size_t j = 0; j < app.size(); j++) { app[j].slot = (int)below(3); app[j].bundle_idx = (uint32_t)below(2); app[j].cache_idx = 50 + (uint32_t)j; app[j].degree = (uint32_t)below(12); }
        const RegistryAfter ra = registry_after(old, dropped, replaced, app);
        CHECK(ra.new_id.size() == k + app.size());
        int next = 0;
        for (size_t i = 0; i < k; i++) {
            if (dropped[i]) { CHECK(ra.new_id[i] == -1); continue; }
            CHECK(ra.new_id[i] == next);
            const RegUnit &u = ra.registry[(size_t)next];
            CHECK(u.slot == old[i].slot && u.bundle_idx == old[i].bundle_idx && u.cache_idx == old[i].cache_idx);
            CHECK(u.degree == (replaced[i] >= 0 ? (uint32_t)replaced[i] : old[i].degree));
            next++;
        }
        for (size_t j = 0; j < app.size(); j++) { CHECK(ra.new_id[k + j] == next); CHECK(ra.registry[(size_t)next].cache_idx == app[j].cache_idx); next++; }
        CHECK(ra.registry.size() == (size_t)next);
        (void)device_loads(ra.registry, 3);
        registries++;
    }
    {
        std::vector<RegUnit> two(2);
        two[0].cache_idx = two[1].cache_idx = 4;
        CHECK(refuses([&] { index_in_cache_order(two, 0); }));
        two[1].bundle_idx = 1;
        CHECK(index_in_cache_order(two, 0).size() == 1 && index_in_cache_order(two, 2).empty());
        CHECK(refuses([&] { registry_after(two, { 1, 0 }, { 3, -1 }, {}); }));
        CHECK(refuses([&] { registry_after(two, { 1 }, { -1, -1 }, {}); }));
        CHECK(refuses([&] { registry_after(two, { 0, 0 }, { -1 }, {}); }));
        CHECK(refuses([&] { merge_first({}); }));
        const RegistryAfter all_gone = registry_after(two, { 1, 1 }, { -1, -1 }, {});
        CHECK(all_gone.registry.empty() && all_gone.new_id == std::vector<int>({ -1, -1 }));
    }
    std::printf("%zu units placed, %zu registries renumbered\nok\n", placed, registries);
    return 0;
}
