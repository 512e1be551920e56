// The arithmetic of the BinBundle update (Engine::update_bundle, k_bins_update), as functions of one lane's values: no HIP in here.
// The kernel runs them with wave shuffles in between, the CPU emulation (emu/db.cpp: emu_bin_update) with an explicit loop over the
// 64 lanes, so the scan and the carry between register slots can be stepped through where a debugger reaches them
// (tests/test_bundle_update_cpu.py).
//
// A bin's polynomial P = sum p_i x^i mod t lives as in k_polyn_with_roots: coefficient i in lane i % 64, register slot i / 64.
//   insert r:  P <- P (x - r):   p'_i = p_{i-1} - r p_i                                   (one lane shift, one multiply-add)
//   remove r:  P <- P / (x - r): synthetic division, q_{k-1} = p_k + r q_k from the top coefficient down, remainder p_0 + r q_0.
// With s_k = p_k + r s_{k+1} (s above the top coefficient = 0) the quotient is q_{k-1} = s_k and the remainder s_0.  Each step is the
// affine map f_k(x) = p_k + r x, held as the pair (m, v) = (r, p_k) meaning x -> v + m x; maps compose associatively,
//   (m2, v2) o (m1, v1) = (m1 m2, v2 + m2 v1)          ((m1, v1) applied first),
// so a slot's 64 maps are combined by a suffix scan over the lanes in 6 steps (lane l takes the pair of lane l + d, d = 1, 2, .. 32,
// as the map applied BEFORE its own; nothing beyond lane 63), and the value entering a slot from above -- s at lane 0 of the next
// slot -- is pushed through the scanned pair of every lane: s = v + m * carry.
#pragma once
#include "modmath.h"

namespace apsu_he {

constexpr int BIN_LANES = 64;

struct ScanPair {
    u64 m, v;                                              // the map x -> v + m x  (mod t)
};

// P'[i] = P[i-1] - r P[i], neg_r = t - r (0 for r = 0)
HD u64 bin_insert_step(u64 p_i, u64 p_below, u64 neg_r, const Mod &t) { return addmod(mulmod(p_i, neg_r, t), p_below, t.q); }

// outer o inner: inner is applied first
HD ScanPair bin_scan_compose(const ScanPair &outer, const ScanPair &inner, const Mod &t)
{
    return ScanPair{ mulmod(inner.m, outer.m, t), addmod(outer.v, mulmod(outer.m, inner.v, t), t.q) };
}

// the slot-carry rule: what a lane's scanned pair makes of the value that enters its slot from the slot above
HD u64 bin_scan_carry(const ScanPair &p, u64 carry, const Mod &t) { return addmod(p.v, mulmod(p.m, carry, t), t.q); }

// The stored residue mod q_0 of a plaintext coefficient back to its value mod t.  The lift (k_lift) leaves v < (t + 1) / 2 alone and
// stores v + (q_0 - t) otherwise; SEAL's monomial shortcut stores v itself whatever its size.  q_0 > 2 t keeps the two ranges apart:
// a lifted value is at least q_0 - t + (t + 1) / 2 > t.
HD u64 bin_unlift(u64 x, u64 t, u64 q0) { return x < t ? x : x - (q0 - t); }

// first bin (lowest slot) and position in its removal list of a root that did not divide, as one word for atomicMin
HD u64 bin_fail_word(u32 bin, u32 pos) { return ((u64)bin << 32) | pos; }

}  // namespace apsu_he
