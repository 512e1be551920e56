// What a resident BinBundle answers to a query, in plaintext (Engine::bundles_eval_plain, Engine::self_test, k_bins_eval, k_eval_compare):
// the arithmetic of one lane and the pure host functions, no HIP in here.  With poly[d][slot] the decoded array of a BinBundle
// (Engine::decode_bundle; rows above a slot's count are 0) the querier who sent x decrypts, in slot s,
//   out[s] = P_s(x[s]) + mask[s]  mod t,   P_s = the column s,
// one point per slot.  The kernels run the lane functions below, the CPU emulation (emu/db.cpp: emu_bins_eval) the same loop
// structure with an explicit loop over the 64 lanes (tests/test_bundle_eval_cpu.py).
//
// k_bins_eval has lane = slot: a wave owns a tile of 64 consecutive slots and walks the rows d = top .. 0, one contiguous 512-byte row
// segment per d, EVAL_ROWS segments in flight (loads first, then their Horner steps) -- no lane walks down a column, the rule of
// k_bins_lookup.  `top` is the tile's largest count, the maximum over the wave of k_bin_counts' output, so a tile of short bins does
// not pay for the BinBundle's longest bin; a tile without a bin reads nothing.  A slot that holds the zero polynomial is not a bin: its
// sum stays 0 and it yields mask[s] alone, which is what the homomorphic evaluation yields there.
//
// One Horner step is  acc x + p  reduced once, with the unreduced multiply-add of bin_merge.h in its two widths:
//   bits(t) <= 32: one 64-bit word -- (2^32 - 1)^2 + (2^32 - 1) < 2^64, the case F = 1 of merge_fold_exact;
//   otherwise:     128 bits (mac128 / barrett128), up to the 60 bits a context accepts.
// Every value that enters or leaves a step is a canonical residue.
#pragma once
#include <cstddef>
#include <cstdint>

#include "bin_merge.h"

namespace apsu_he {

constexpr int EVAL_LANES = 64;
constexpr int EVAL_ROWS = 8;                              // row segments in flight per wave of k_bins_eval (resource report: profiles/r17_self_test.txt)
static_assert(merge_fold_interval(32) >= 1 && merge_fold_interval(MERGE_MAX_PLAIN_BITS) >= 1, "one multiply-add on top of a residue fits the sum");

// acc <- acc x + p  (mod t); acc, x, p < t
template <bool NARROW> HD u64 eval_step(u64 acc, u64 x, u64 p, const Mod &t)
{
    if (NARROW) {
        u64 s = p;
        merge_mac_narrow(s, acc, x);
        return merge_fold_narrow(s, t);
    }
    u128p s{ p, 0 };
    merge_mac_wide(s, acc, x);
    return merge_fold_wide(s, t);
}

// one lane's walk: rows d = top .. 0 of its column (stride n words), EVAL_ROWS loads before their steps; top < 0: nothing is read
template <bool NARROW> HD u64 eval_walk(const u64 *col, size_t n, int top, u64 x, const Mod &t)
{
    u64 acc = 0;
    int d = top;
    for (; d >= EVAL_ROWS - 1; d -= EVAL_ROWS) {
        u64 p[EVAL_ROWS];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int k = 0; k < EVAL_ROWS; k++) p[k] = col[(size_t)(d - k) * n];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int k = 0; k < EVAL_ROWS; k++) acc = eval_step<NARROW>(acc, x, p[k], t);
    }
    for (; d >= 0; d--) acc = eval_step<NARROW>(acc, x, col[(size_t)d * n], t);
    return acc;
}

// the closing addition of the slot's mask value (< t)
HD u64 eval_finish(u64 acc, u64 mask, const Mod &t) { return addmod(acc, mask, t.q); }

// a slot's count as the top of its own walk: -1 for a slot that is not a bin; the tile's top is the largest over its 64 lanes
HD int eval_count_top(u32 count) { return count == LOOKUP_NONE ? -1 : (int)count; }
HD bool eval_is_bin(u32 count) { return count != LOOKUP_NONE; }
// the walk is d = eval_walk_top(..) .. 0 (none for -1): never above the array's last row, whatever the counts say
HD int eval_walk_top(int tile_top, u32 rows) { return tile_top < (int)rows ? tile_top : (int)rows - 1; }

// ---- the self-test's comparison (k_eval_compare): one lane per (BinBundle, slot); FIRST = the lowest (position << 32 | slot) that differs
constexpr u64 EVAL_NO_MISMATCH = ~(u64)0;
HD u64 eval_mismatch_key(u32 position, u32 slot) { return (u64)position << 32 | slot; }

// what the self-test reports (include/apsu_he.h: apsu_he_self_test_report has the same fields in the same order)
struct SelfTestReport {
    uint32_t bundles, reserved;
    uint64_t slots, mismatches;
    int32_t first_bundle;                                 // position in the call's list (the BinBundle's id on a multi-device handle), -1: none
    uint32_t first_slot;
    uint64_t first_got, first_expected;
    int32_t min_budget_bits, min_budget_bundle;           // the smallest noise budget and the first BinBundle that has it (-1: nothing checked)
    double he_ms, plain_ms;
};

inline SelfTestReport self_test_empty()
{
    SelfTestReport r{};
    r.first_bundle = -1;
    r.min_budget_bundle = -1;
    return r;
}

// Reports of disjoint parts of one database -> the report of the whole.  Every part names BinBundles by their position in the whole
// (a multi-device handle: by id), so the first mismatch is the lowest (position, slot) and the smallest budget goes to the lowest
// position that has it.  The parts ran side by side: the times are the slowest part's.
inline void self_test_reduce(SelfTestReport &into, const SelfTestReport &part)
{
    into.bundles += part.bundles;
    into.slots += part.slots;
    into.mismatches += part.mismatches;
    if (part.first_bundle >= 0 &&
        (into.first_bundle < 0 || eval_mismatch_key((u32)part.first_bundle, part.first_slot) < eval_mismatch_key((u32)into.first_bundle, into.first_slot))) {
        into.first_bundle = part.first_bundle; into.first_slot = part.first_slot;
        into.first_got = part.first_got; into.first_expected = part.first_expected;
    }
    if (part.min_budget_bundle >= 0 &&
        (into.min_budget_bundle < 0 || part.min_budget_bits < into.min_budget_bits ||
         (part.min_budget_bits == into.min_budget_bits && part.min_budget_bundle < into.min_budget_bundle))) {
        into.min_budget_bits = part.min_budget_bits; into.min_budget_bundle = part.min_budget_bundle;
    }
    if (part.he_ms > into.he_ms) into.he_ms = part.he_ms;
    if (part.plain_ms > into.plain_ms) into.plain_ms = part.plain_ms;
}

// The self-test's own draws from the Blake2xb stream of its seed, as 32-bit outputs (16 per 64-byte stream block) reduced mod t like
// the masks of apsu_he_mask_generate_blake2xb.  query_side.h assigns blocks below 2^21 + 2^20 * 4096 < 2^33; the self-test takes
//   slot values of the i-th distinct bundle index:  outputs 2^37 + i n + [0, n)      (blocks from 2^33)
//   mask values of the BinBundle at position p:     outputs 2^38 + p n + [0, n)      (blocks from 2^34)
// n <= 32768 and fewer than 2^20 of either keep both inside their 2^33 blocks.
constexpr u64 SELF_TEST_X_FIRST = (u64)1 << 37;
constexpr u64 SELF_TEST_MASK_FIRST = (u64)1 << 38;
constexpr u64 SELF_TEST_MAX_OBJECTS = (u64)1 << 20;

}  // namespace apsu_he
