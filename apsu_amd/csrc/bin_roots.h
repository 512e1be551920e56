// Reading a resident BinBundle's bins back from its polynomials (Engine::bundle_bins, k_bin_roots, k_roots_mult): the rules and the
// arithmetic of one lane, no HIP in here.  The kernels (kernels_roots.hip) run these functions on the GPU, the CPU emulation
// (emu/roots.cpp: emu_bin_roots) steps them over the lanes of a workgroup (tests/test_bundle_roots_cpu.py).
//
// Batching forces t = 1 (mod 2n).  The forward negacyclic transform mod t evaluates a polynomial of degree below n at the n points
// psi^odd, one coset psi <w> of the subgroup <w> of order n of F_t^*.  Scaling coefficient i by c^i moves the evaluation to the coset
// c psi <w>, and with c_j = g^j for a generator g of F_t^*, j < (t - 1) / n, the cosets tile F_t^* exactly once.  So the roots of a
// bin's polynomial P are the zeros of (t - 1) / n transforms of (a_i c_j^i)_i, plus the root 0 (which lies in no coset) iff a_0 = 0.
//   the walk:    v_i = a_i c_j^i;  between consecutive cosets v_i <- v_i g^i  (step table g^i, i < n)
//   the points:  output position k of coset j is the value at c_j pts[k], pts = the forward transform of the polynomial X -- the
//                transform's output order is never re-derived
//   the multiplicity of a found root r: the first Hasse derivative P'(r) by a two-accumulator Horner walk tells whether r is a
//                multiple root at all; only then the bin's polynomial is divided by (x - r) as long as the remainder is 0
// Everything here needs t < 2^32, which the bound on the coset count gives for every ring size the engine has (t <= 2^16 n + 1).
#pragma once
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "ntt_core.h"

namespace apsu_he {

constexpr u32 ROOTS_MAX_COSETS = 65536;                          // a condition of the call ((t - 1) / n above it: APSU_HE_LOGIC_ERROR)
constexpr int ROOTS_LANES = 64;

// a b mod q for a, b < 2^32 (the product fits one word; r1 = floor(2^64 / q), the quotient estimate is short by at most 1)
HD u64 roots_mul(u64 a, u64 b, u64 q, u64 r1)
{
    const u64 x = a * b, v = x - mulhi64(x, r1) * q;
    return v >= q ? v - q : v;
}
HD u64 roots_pow(u64 b, u64 e, u64 q, u64 r1)
{
    u64 r = 1;
    for (; e; e >>= 1) {
        if (e & 1) r = roots_mul(r, b, q, r1);
        b = roots_mul(b, b, q, r1);
    }
    return r;
}

// ---- the lane functions both tiers run
// the scaled load: a_i c^i (the first coset of a workgroup's range); the step between consecutive cosets: v_i g^i
HD u64 roots_scaled_load(u64 a, u64 c, u32 i, u64 q, u64 r1) { return roots_mul(a, roots_pow(c, i, q, r1), q, r1); }
HD u64 roots_step(u64 v, u64 g_i, u64 q, u64 r1) { return roots_mul(v, g_i, q, r1); }
// the scaling of the coset in FRONT of coset j0, so that a workgroup's every transform (the first included) starts with a step:
// g^(j0 - 1), exponents mod t - 1
HD u64 roots_coset_before(u64 g, u32 j0, u64 q, u64 r1) { return roots_pow(g, ((u64)j0 + q - 2) % (q - 1), q, r1); }
// the zero test of output position k of coset c, with its append of the value to the bin's list: `list` has room for `cap` values
// (the bin's count: a polynomial has no more roots than its degree), *found counts the appends
HD bool roots_is_zero(u64 y) { return y == 0; }
HD u64 roots_value(u64 c, u64 pt, u64 q, u64 r1) { return roots_mul(c, pt, q, r1); }
HD void roots_append(u32 *found, u64 *list, u32 cap, u64 value)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const u32 at = atomicAdd(found, 1u);
#else
    const u32 at = (*found)++;
#endif
    if (at < cap) list[at] = value;
}
// P(r) and the first Hasse derivative P'(r), coefficient a from the top down: (b0, b1) <- (b0 r + a, b1 r + b0)
HD void roots_deriv_step(u64 &b0, u64 &b1, u64 r, u64 a, u64 q, u64 r1)
{
    b1 = addmod(roots_mul(b1, r, q, r1), b0, q);
    b0 = addmod(roots_mul(b0, r, q, r1), a, q);
}
// synthetic division by (x - r) from the top coefficient down: s <- p_k + r s; the quotient's coefficient k - 1 is s, the remainder
// the last s (bin_update.h has the same step as a scan over a wave)
HD u64 roots_div_step(u64 p_k, u64 r, u64 s, u64 q, u64 r1) { return addmod(p_k, roots_mul(r, s, q, r1), q); }

// ---- the source of the workgroup transform (ntt_wg.h, next to SrcPlain and SrcTensor): the bin's scaled coefficients v[n] (32-bit
// words, LDS on the GPU), stepped to the next coset by the load itself.  Every coefficient is loaded exactly once per transform.
struct SrcCoset { u32 *v; const u32 *step; };

// ---- host rules
inline u64 field_generator(u64 t)
{
    if (t < 3 || (t >> 32)) throw std::logic_error("field_generator: modulus out of range");
    std::vector<u64> primes;
    u64 m = t - 1;
    for (u64 p = 2; p * p <= m; p++)
        if (m % p == 0) {
            primes.push_back(p);
            while (m % p == 0) m /= p;
        }
    if (m > 1) primes.push_back(m);
    const u64 r1 = (u64)((((unsigned __int128)1) << 64) / t);
    for (u64 g = 2; g < t; g++) {
        bool ok = true;
        for (u64 p : primes)
            if (roots_pow(g, (t - 1) / p, t, r1) == 1) { ok = false; break; }
        if (ok) return g;
    }
    throw std::logic_error("field_generator: " + std::to_string(t) + " is not a prime");
}

// the number of cosets, (t - 1) / n; refuses what the walk cannot serve
inline u32 roots_coset_count(u64 t, u64 n)
{
    if (!n || (t - 1) % (2 * n)) throw std::logic_error("plain_modulus does not support batching");
    const u64 cosets = (t - 1) / n;
    if (cosets > ROOTS_MAX_COSETS)
        throw std::logic_error("plain_modulus " + std::to_string(t) + " has " + std::to_string(cosets) + " cosets of the transform's points, more than " +
                               std::to_string(ROOTS_MAX_COSETS) + ": the bins cannot be read back");
    return (u32)cosets;
}

inline std::vector<u32> roots_step_table(u64 g, u64 t, size_t n)
{
    const u64 r1 = (u64)((((unsigned __int128)1) << 64) / t);
    std::vector<u32> s(n);
    u64 x = 1;
    for (size_t i = 0; i < n; i++) { s[i] = (u32)x; x = roots_mul(x, g, t, r1); }
    return s;
}

// The grid of k_bin_roots: work item = (occupied bin, block of consecutive cosets).  One block per bin unless the bins alone leave
// workgroup slots idle; then the cosets are split until there are about four work items per slot, so that the last wave of work
// items is short against the whole.
struct RootsGrid { u32 blocks, per_block; };
inline RootsGrid roots_grid(u32 n_occupied, u32 cosets, u32 wg_slots)
{
    RootsGrid g{ 1, cosets };
    if (!n_occupied || !cosets) return g;
    const u64 want = (u64)4 * wg_slots;
    u32 blocks = (u32)std::min<u64>(cosets, (want + n_occupied - 1) / n_occupied);
    if (blocks < 1) blocks = 1;
    g.per_block = (cosets + blocks - 1) / blocks;
    g.blocks = (cosets + g.per_block - 1) / g.per_block;
    return g;
}

// Host end of the call: bin `slot` with `count` items, the distinct values found and their multiplicities -> the sorted multiset, or
// the refusal (a polynomial that is not a product of linear factors)
inline void roots_expand(u32 slot, u32 count, const u64 *values, const u32 *mult, u32 found, std::vector<u64> &out)
{
    out.clear();
    u64 total = 0;
    for (u32 i = 0; i < found && i < count; i++) total += mult[i];
    if (found > count || total != count)
        throw std::invalid_argument("bin " + std::to_string(slot) + ": its polynomial of degree " + std::to_string(count) + " does not split into linear factors (" +
                                    std::to_string(found > count ? (u64)found : total) + " roots found, counted with multiplicity)");
    for (u32 i = 0; i < found; i++) out.insert(out.end(), mult[i], values[i]);
    std::sort(out.begin(), out.end());
}

}  // namespace apsu_he

// the loads of SrcCoset, where ntt_core.h's passes look for them (next to SrcPlain's)
HD u64x2 src_load2(const apsu_he::SrcCoset &s, const u64 *, int e, const NttTable &tab)
{
    u64x2 r;
    r[0] = apsu_he::roots_step(s.v[e], s.step[e], tab.q, tab.r1);
    r[1] = apsu_he::roots_step(s.v[e + 1], s.step[e + 1], tab.q, tab.r1);
    s.v[e] = (u32)r[0];
    s.v[e + 1] = (u32)r[1];
    return r;
}
HD u64 src_load1(const apsu_he::SrcCoset &s, const u64 *, int e, const NttTable &tab)
{
    const u64 r = apsu_he::roots_step(s.v[e], s.step[e], tab.q, tab.r1);
    s.v[e] = (u32)r;
    return r;
}
HD u64 src_in_bound(const apsu_he::SrcCoset &, const NttTable &) { return 1; }
