// Merging the BinBundles of one bundle index (Engine::merge_bundles, k_bins_merge): the arithmetic of one lane and the pure host
// functions, no HIP in here.  The union of two bins is the product of their polynomials, so with A[dA + 1][n] and B[dB + 1][n] the
// decoded arrays of two BinBundles (Engine::decode_bundle; rows above a slot's count are 0) the merged one is, per slot s,
//   C[k][s] = sum_{i + j = k} A[i][s] B[j][s]  mod t,   k <= dA + dB.
// The kernel runs the lane functions below, the CPU emulation (emu/db.cpp: emu_bins_merge) the same loop structure with an explicit
// loop over the 64 lanes (tests/test_bundle_merge_cpu.py).
//
// k_bins_merge has lane = slot: a wave owns a tile of 64 consecutive slots and a block of MERGE_K consecutive output rows
// k0 .. k0 + K - 1 (k0 a multiple of K), held as K accumulators.  It walks i over A's rows; step i takes the row segment A[i] and
// needs B[k0 + j - i] for j < K: a window of K consecutive rows of B that slides down by one row per step, so one new row B[k0 - i]
// per step.  Row r of B is kept in window slot r mod K; the walk starts at a multiple of K and is unrolled K times, which makes
// every slot index a compile-time constant: acc[j] += A[i] win[(j - u) mod K] at step i = ib + u, and the new row goes to slot
// (K - u) mod K, whose previous row k0 - i + K was used last at step i - 1.  Rows outside 0 .. top are taken as 0 without a load, and
// the tops are the tile's largest counts (merge_tile_tops), so a tile of short bins does not pay for the BinBundle's longest bin.
//
// Lazy accumulation.  The products are summed unreduced and an accumulator is reduced ("folded") once per fold interval:
//   bits(t) <= 32 (t < 2^32): one 64-bit word, every product a 32 x 32 -> 64 multiply-add;
//   otherwise:                128 bits (mac128).
// A product of two values < t is at most (2^b - 1)^2 with b = bits(t), and a folded accumulator re-enters as a value < t, so
// F = 2^(W - 2 b) steps between two folds keep  F (2^b - 1)^2 + 2^b - 1 = 2^W - 2^(W-b+1) + 2^(W-2b) + 2^b - 1  below 2^W
// (W = 64 or 128; the two positive terms are each below half the negative one for b <= 32, W = 64 and for 33 <= b <= 63, W = 128).
// The interval is capped at MERGE_FOLD_CAP: a fold per 1024 steps costs nothing, and it keeps the step counter and the chains a test
// has to build short.  The count is of STEPS of the walk (a step adds one product to each accumulator), whether or not the step's
// rows were inside the tops.  merge_fold_exact checks the bound itself in 128-bit arithmetic for every width a context accepts.
#pragma once
#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

#include "bin_lookup.h"

namespace apsu_he {

constexpr int MERGE_LANES = 64;
constexpr int MERGE_K = 8;                                // output rows per wave of k_bins_merge (resource report: profiles/r11_bundle_merge.txt)
constexpr u32 MERGE_FOLD_CAP = 1024;
constexpr int MERGE_MAX_PLAIN_BITS = 60;                  // SEAL_USER_MOD_BIT_COUNT_MAX: the widest plain modulus a context accepts

constexpr int merge_bits(u64 t) { int b = 0; while (t) { b++; t >>= 1; } return b; }
constexpr bool merge_narrow(int bits) { return bits <= 32; }          // the sum lives in one 64-bit word
constexpr u32 merge_fold_interval(int bits)
{
    const int w = (merge_narrow(bits) ? 64 : 128) - 2 * bits;         // >= 0 for bits <= 32 and for 33 .. 64
    return w >= 10 ? MERGE_FOLD_CAP : (u32)1 << w;
}

// F (2^b - 1)^2 + (2^b - 1) fits the accumulator: neither the product nor the sum wraps
constexpr bool merge_fold_exact(int bits)
{
    const unsigned __int128 m = ((unsigned __int128)1 << bits) - 1, F = merge_fold_interval(bits);
    if (merge_narrow(bits)) return F * m * m + m <= (unsigned __int128)~(u64)0;
    // 128-bit sums: F m m < 2^(w + 2 b) <= 2^128 cannot be tested after the fact, so test the factors: F <= floor((2^128 - 1 - m) / m / m)
    const unsigned __int128 all = ~(unsigned __int128)0;
    return F <= (all - m) / m / m;
}
constexpr bool merge_fold_exact_all()
{
    for (int b = 1; b <= MERGE_MAX_PLAIN_BITS; b++)
        if (!merge_fold_exact(b)) return false;
    return true;
}
static_assert(merge_fold_exact_all(), "k_bins_merge: the fold interval overflows the lazy sum for some plain modulus width");
static_assert(MERGE_K >= 1 && MERGE_K <= 16, "MERGE_K");

// one step of one accumulator, and its fold
HD void merge_mac_narrow(u64 &acc, u64 a, u64 b) { acc += (u64)(u32)a * (u32)b; }
HD void merge_mac_wide(u128p &acc, u64 a, u64 b) { mac128(acc, a, b); }
HD u64 merge_fold_narrow(u64 acc, const Mod &t) { return barrett64(acc, t); }
HD u64 merge_fold_wide(u128p acc, const Mod &t) { return barrett128(acc, t); }

// the walk of one (tile, row block): steps i = i0 .. i1 (none when i1 < i0), i0 a multiple of K.  topA / topB: the tile's largest
// counts, -1 where the tile has no bin.  Only steps with i <= topA and 0 <= k0 + j - i <= topB for some j < K can add anything.
struct MergeWalk { int i0, i1; };
HD MergeWalk merge_walk(int k0, int K, int topA, int topB)
{
    if (topA < 0 || topB < 0 || k0 > topA + topB) return MergeWalk{ 0, -1 };
    const int lo = k0 - topB > 0 ? k0 - topB : 0, hi = k0 + K - 1 < topA ? k0 + K - 1 : topA;
    return MergeWalk{ lo / K * K, hi };
}

// per tile of 64 slots the largest count, -1 for a tile without a bin (counts: LOOKUP_NONE = not a bin)
inline std::vector<int> merge_tile_tops(const u32 *counts, size_t n)
{
    std::vector<int> tops((n + MERGE_LANES - 1) / MERGE_LANES, -1);
    for (size_t s = 0; s < n; s++)
        if (counts[s] != LOOKUP_NONE && (int)counts[s] > tops[s / MERGE_LANES]) tops[s / MERGE_LANES] = (int)counts[s];
    return tops;
}

// What may be merged: the two inputs have the same set of bins (a slot that holds the zero polynomial in exactly one of them is an
// error; in both it stays the zero polynomial), and with max_items != 0 no summed count reaches max_items -- the placement rule's
// strict bound (db_place.h).  sum[s] = the merged counts.  The first offending slot is named: std::invalid_argument.
inline void merge_counts(const u32 *a, const u32 *b, size_t n, u32 max_items, u32 *sum)
{
    for (size_t s = 0; s < n; s++) {
        if ((a[s] == LOOKUP_NONE) != (b[s] == LOOKUP_NONE))
            throw std::invalid_argument("slot " + std::to_string(s) + " is a bin in one BinBundle and holds the zero polynomial in the other");
        if (a[s] == LOOKUP_NONE) { sum[s] = LOOKUP_NONE; continue; }
        const u64 c = (u64)a[s] + b[s];
        if (max_items && c >= max_items)
            throw std::invalid_argument("bin " + std::to_string(s) + ": the merged bin would hold " + std::to_string(c) +
                                        " items, max_items_per_bin - 1 = " + std::to_string(max_items - 1) + " is the most");
        sum[s] = (u32)c;
    }
}

// The host decisions of a merge of n_bundles >= 1 BinBundles (counts [n_bundles][n], degrees [n_bundles]).  Step k < n_bundles - 1
// multiplies the product of BinBundles 0 .. k (counts: the running sums) by BinBundle k + 1:
//   tops[(2 k) tiles ..] and tops[(2 k + 1) tiles ..]: merge_tile_tops of the two operands;
//   rows[k]: the rows k_bins_merge writes = the largest count of either operand, summed, + 1.  The two need not be in the same slot, so
//            rows[k] can exceed the step's degree + 1, and an early step can be the tallest;
//   degree: the largest summed count of all.
// Refusals, step by step and before anything else is decided for that step: merge_counts' (std::invalid_argument), then
// std::logic_error where an operand's largest count exceeds its BinBundle's degree (the decoded array has no such row).
struct MergeSteps { std::vector<u32> rows; std::vector<int> tops; u32 degree = 0; };
inline MergeSteps merge_steps(const u32 *counts, const u32 *degrees, u32 n_bundles, size_t n, u32 max_items)
{
    const size_t tiles = (n + MERGE_LANES - 1) / MERGE_LANES;
    const u32 steps = n_bundles - 1;
    auto top_of = [](const std::vector<int> &t) { int m = 0; for (int v : t) m = v > m ? v : m; return (u32)m; };
    MergeSteps ms;
    ms.rows.resize(steps);
    ms.tops.resize((size_t)2 * steps * tiles);
    std::vector<u32> run(counts, counts + n), next(n);
    for (u32 k = 0; k < steps; k++) {
        const u32 *cb = counts + (size_t)(k + 1) * n;
        merge_counts(run.data(), cb, n, max_items, next.data());
        const std::vector<int> ta = merge_tile_tops(run.data(), n), tb = merge_tile_tops(cb, n);
        if (top_of(tb) > degrees[k + 1] || (!k && top_of(ta) > degrees[0])) throw std::logic_error("merge: a bin count exceeds its BinBundle's degree");
        for (size_t i = 0; i < tiles; i++) { ms.tops[(size_t)2 * k * tiles + i] = ta[i]; ms.tops[(size_t)(2 * k + 1) * tiles + i] = tb[i]; }
        ms.rows[k] = top_of(ta) + top_of(tb) + 1;
        run.swap(next);
    }
    ms.degree = top_of(merge_tile_tops(run.data(), n));
    return ms;
}

}  // namespace apsu_he
