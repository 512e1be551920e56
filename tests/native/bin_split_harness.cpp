// Stand-alone driver of the split's functions (apsu_amd/csrc/bin_split.h: the rules, and k_roots_split as a loop over its work items,
// split_emulate; apsu_amd/csrc/db_rebase.h: rebase_plan), meant to be built with -fsanitize=address,undefined
// (tests/test_bundle_split_cpu.py).  Every array handed over is an exact-size heap allocation, so a read or write past its end is seen:
// the lists hold hstride words per bin and not one more, a part's array ends with its last slot's row.  The expected values are
// std::sort and slicing.  Prints "ok" and returns 0, or says what differed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "bin_split.h"
#include "db_rebase.h"

using namespace apsu_he;

namespace {

[[noreturn]] void fail(const std::string &what)
{
    std::fprintf(stderr, "FAILED: %s\n", what.c_str());
    std::exit(1);
}
#define EXPECT(cond) do { if (!(cond)) fail(std::string(#cond) + " (line " + std::to_string(__LINE__) + ")"); } while (0)

uint64_t next(uint64_t &s) { s += 0x9e3779b97f4a7c15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }

template <class T> std::unique_ptr<T[]> exact(size_t count) { return std::unique_ptr<T[]>(new T[count ? count : 1]); }

constexpr u64 POISON = 0xEEEEEEEEEEEEEEEEull;

// bins: per occupied slot its multiset; the lists are written in a shuffled arrival order, multiplicities only where there is a deficit
void run(u32 n, u32 hstride, u32 k, const std::vector<std::pair<u32, std::vector<u64>>> &bins, uint64_t &seed)
{
    const u32 n_occ = (u32)bins.size();
    auto hits = exact<u64>((size_t)n_occ * hstride);
    auto mult = exact<u32>((size_t)n_occ * hstride);
    auto found = exact<u32>(n_occ), occ = exact<u32>(n_occ), counts = exact<u32>(n);
    for (u32 s = 0; s < n; s++) counts[s] = 0xFFFFFFFFu;
    u32 last_slot = 0;
    for (u32 r = 0; r < n_occ; r++) {
        std::vector<u64> items = bins[r].second, vals;
        std::sort(items.begin(), items.end());
        for (u64 v : items) if (vals.empty() || vals.back() != v) vals.push_back(v);
        for (size_t i = vals.size(); i > 1; i--) std::swap(vals[i - 1], vals[next(seed) % i]);
        occ[r] = bins[r].first; counts[occ[r]] = (u32)items.size(); found[r] = (u32)vals.size();
        last_slot = std::max(last_slot, occ[r]);
        for (u32 i = 0; i < hstride; i++) { hits[(size_t)r * hstride + i] = POISON; mult[(size_t)r * hstride + i] = 0xEEEEEEEEu; }
        for (size_t i = 0; i < vals.size(); i++) {
            hits[(size_t)r * hstride + i] = vals[i];
            if (vals.size() < items.size()) mult[(size_t)r * hstride + i] = (u32)std::count(items.begin(), items.end(), vals[i]);
        }
    }
    // part p: exactly (last occupied slot + 1) rows of exactly the fullest part's width
    auto off = exact<u64>(k);
    auto stride = exact<u32>(k);
    size_t words = 0;
    for (u32 p = 0; p < k; p++) {
        u32 most = 0;
        for (u32 r = 0; r < n_occ; r++) { const u32 c = counts[occ[r]]; most = std::max(most, split_cut(c, k, p + 1) - split_cut(c, k, p)); }
        off[p] = words; stride[p] = most;
        words += (size_t)(last_slot + 1) * most;
    }
    auto out = exact<u64>(words);
    for (size_t i = 0; i < words; i++) out[i] = POISON;
    auto counts_out = exact<u32>((size_t)k * n);
    u64 failure = SPLIT_NO_FAILURE;
    split_emulate(hits.get(), found.get(), mult.get(), hstride, occ.get(), counts.get(), n_occ, k, out.get(), off.get(), stride.get(), counts_out.get(), n, &failure);
    EXPECT(failure == SPLIT_NO_FAILURE);
    std::vector<bool> written(words, false);
    for (u32 r = 0; r < n_occ; r++) {
        std::vector<u64> items = bins[r].second;
        std::sort(items.begin(), items.end());
        const u32 c = (u32)items.size(), s = occ[r];
        for (u32 p = 0; p < k; p++) {
            const u32 lo = split_cut(c, k, p), hi = split_cut(c, k, p + 1);
            EXPECT(counts_out[(size_t)p * n + s] == hi - lo);
            for (u32 i = lo; i < hi; i++) {
                const size_t at = off[p] + (size_t)s * stride[p] + (i - lo);
                EXPECT(out[at] == items[i]);
                written[at] = true;
            }
        }
    }
    for (size_t i = 0; i < words; i++) EXPECT(written[i] || out[i] == POISON);
    for (u32 p = 0; p < k; p++)
        for (u32 s = 0; s < n; s++)
            if (counts[s] == 0xFFFFFFFFu) EXPECT(counts_out[(size_t)p * n + s] == 0);
}

}  // namespace

int main()
{
    uint64_t seed = 42;
    // the rules
    for (u32 c = 0; c <= 70; c++)
        for (u32 k = 1; k <= 80; k++) {
            EXPECT(split_cut(c, k, 0) == 0 && split_cut(c, k, k) == c);
            for (u32 pos = 0; pos < c; pos++) { const u32 p = split_part_of(c, k, pos); EXPECT(p < k && split_cut(c, k, p) <= pos && pos < split_cut(c, k, p + 1)); }
        }
    EXPECT(split_cut(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFEu) == 0xFFFFFFFEu);      // no 32-bit overflow in p c
    EXPECT(split_part_of(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFEu) == 0xFFFFFFFEu);
    for (u32 c = 0; c <= 300; c++)
        for (u32 limit = 2; limit <= 130; limit++) { const u32 k = split_parts(c, limit); EXPECT((c + k - 1) / k < limit && (k == 1 || (c + k - 2) / (k - 1) >= limit)); }
    // the kernel as a loop, every instance at and around its capacity
    for (u32 h : { 1u, 5u, 255u, 256u, 257u, 2048u, 2049u, 8192u })
        for (u32 k : { 1u, 2u, 3u, 7u }) {
            std::vector<std::pair<u32, std::vector<u64>>> bins;
            std::vector<u64> full, rep;
            for (u32 i = 0; i < h; i++) full.push_back((next(seed) % 4000000000ull));
            for (u32 i = 0; i < h; i++) rep.push_back(next(seed) % 7);
            bins.push_back({ 0, full });
            bins.push_back({ 3, rep });
            bins.push_back({ 9, std::vector<u64>(std::min(h, 5u), 0xFFFFFFFEull) });      // one root of multiplicity c, the widest value
            bins.push_back({ 10, { 0 } });
            run(11, h, k, bins, seed);
        }
    // rebase_plan
    const u32 mc[4] = { 227, 0, 127, 500 }, bi[4] = { 1, 1, 0, 1 };
    const RebasePlan plan = rebase_plan(mc, bi, 4, 128);
    EXPECT(plan.parts == (std::vector<u32>{ 2, 1, 1, 4 }) && plan.cache_idx == (std::vector<u32>{ 0, 1, 2, 0, 3, 4, 5, 6 }));
    EXPECT(plan.origin == (std::vector<u32>{ 0, 0, 1, 2, 3, 3, 3, 3 }) && plan.first == (std::vector<u32>{ 0, 2, 3, 4 }));
    std::puts("ok");
    return 0;
}
