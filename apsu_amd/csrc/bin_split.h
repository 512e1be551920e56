// Splitting the bins of a resident BinBundle (Engine::split_bundle, k_roots_split): the rules and the arithmetic of one work item, no HIP
// in here.  The kernel (kernels_roots.hip) runs these functions on the GPU, the CPU emulation (emu/roots.cpp: emu_roots_split) steps them
// over the work items of a workgroup (tests/test_bundle_split_cpu.py).
//
// The contract of a split into k parts.  A bin holds the sorted multiset r_0 <= ... <= r_{c-1}; part p holds the positions
// [split_cut(c, k, p), split_cut(c, k, p + 1)) of it, split_cut(c, k, p) = floor(p c / k).  So every part of every bin has floor(c / k)
// or ceil(c / k) items, equal values may straddle a cut (the parts are multisets), an empty bin is empty in every part, and a slot that
// is not a bin is not a bin in any part.
//
// What the kernel starts from is what the root search leaves on the device (launch_roots.h): per occupied bin the DISTINCT roots in the
// order the atomics appended them, and their multiplicities.  One workgroup per bin:
//   keys:   value << 32 | multiplicity (t < 2^32 is the root search's own condition), padded to the instance's capacity, a power of two,
//           with SPLIT_SENTINEL, which sorts behind every key
//   sort:   a bitonic network over the capacity; pass (size, j) exchanges the pairs split_pair(i, j), i < capacity / 2, ascending where
//           split_ascending(lo, size)
//   scan:   every work item owns capacity / work items consecutive keys; an exclusive scan of the multiplicities (split_combine) gives each distinct
//           root the position of its first copy in the sorted multiset, and the total
//   check:  the total is the bin's count and there are no more distinct roots than items, else the bin's polynomial is not a product of
//           linear factors: split_failure(slot, what was found), the smallest of which the call reports (roots_expand's refusal)
//   write:  copy q of a root at first position pos goes to position pos + q of the multiset, which part split_part_of(c, k, pos + q) owns
#pragma once
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "ntt_core.h"

namespace apsu_he {

constexpr u64 SPLIT_SENTINEL = ~(u64)0;                          // no key: a value is below t < 2^32
constexpr u64 SPLIT_NO_FAILURE = ~(u64)0;                        // the failure word beforehand
constexpr u32 SPLIT_CAP_SMALL = 256, SPLIT_CAP_MID = 2048, SPLIT_CAP_LARGE = 8192;
// work items of the instance of a capacity; each owns capacity / work items consecutive keys in the scan (4, 8, 8)
HD u32 split_threads(u32 capacity) { return capacity == SPLIT_CAP_SMALL ? 64 : capacity == SPLIT_CAP_MID ? 256 : 1024; }
constexpr u32 SPLIT_MULT_MAX = (u32)1 << 18;                     // a multiplicity's bound by contract: capacity * bound < 2^32

HD u32 split_cut(u32 c, u32 k, u32 p) { return (u32)((u64)p * c / k); }
// the part that owns position pos < c: the largest p with split_cut(c, k, p) <= pos
HD u32 split_part_of(u32 c, u32 k, u32 pos) { return (u32)((((u64)pos + 1) * k - 1) / c); }
// the instance for lists of up to hstride distinct roots: its capacity in keys, 0 for none
HD u32 split_capacity(u32 hstride) { return hstride <= SPLIT_CAP_SMALL ? SPLIT_CAP_SMALL : hstride <= SPLIT_CAP_MID ? SPLIT_CAP_MID : hstride <= SPLIT_CAP_LARGE ? SPLIT_CAP_LARGE : 0; }

HD u64 split_key(u64 value, u32 mult) { return value << 32 | mult; }
HD u64 split_key_value(u64 key) { return key >> 32; }
HD u32 split_key_mult(u64 key) { return key == SPLIT_SENTINEL ? 0 : (u32)key; }
// entry i of a bin's list as the kernel loads it: a key below min(found, count), the sentinel behind; the multiplicities are read only
// where the bin has fewer distinct roots than items (launch_roots_mult writes no others)
HD u64 split_load(const u64 *hits, const u32 *mult, u32 i, u32 found, u32 count)
{
    if (i >= found || i >= count) return SPLIT_SENTINEL;
    return split_key(hits[i], found < count ? mult[i] : 1);
}
// pair i of the pass with distance j (a power of two): lo has bit j clear, hi = lo + j
HD void split_pair(u32 i, u32 j, u32 &lo, u32 &hi)
{
    lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
    hi = lo | j;
}
HD bool split_ascending(u32 lo, u32 size) { return (lo & size) == 0; }
HD void split_exchange(u64 &a, u64 &b, bool ascending)
{
    if ((a > b) == ascending) { const u64 x = a; a = b; b = x; }
}
HD u32 split_combine(u32 a, u32 b) { return a + b; }
// the word a failing bin reports; the smallest over the bins names the first such slot
HD u64 split_failure(u32 slot, u32 found, u32 count, u32 total) { return (u64)slot << 32 | (found > count ? found : total); }
HD bool split_bin_ok(u32 found, u32 count, u32 total) { return found <= count && total == count; }
// the copies of one distinct root: positions pos .. pos + mult - 1 of a bin of c items, each into its part's row of the bin.  out: the
// parts' arrays in one buffer, part p at out + part_off[p] with part_stride[p] words per slot.
HD void split_write(u64 *out, const u64 *part_off, const u32 *part_stride, u32 slot, u32 c, u32 k, u32 pos, u32 mult, u64 value)
{
    if (!mult) return;
    u32 p = split_part_of(c, k, pos), lo = split_cut(c, k, p), hi = split_cut(c, k, p + 1);
    for (u32 q = pos; q < pos + mult; q++) {
        while (q >= hi) { p++; lo = hi; hi = split_cut(c, k, p + 1); }
        out[part_off[p] + (size_t)slot * part_stride[p] + (q - lo)] = value;
    }
}

// ---- the kernel as a loop (host only): launch_roots_split's arguments on host arrays, the workgroups one after the other, every work
// item of a workgroup stepped through the functions above in the kernel's order, the zeroing of counts_out included.  *failure:
// SPLIT_NO_FAILURE beforehand.  Throws for what the launcher refuses.
inline void split_emulate(const u64 *hits, const u32 *found, const u32 *mult, u32 hstride, const u32 *occ, const u32 *counts, u32 n_occ, u32 k, u64 *out,
                          const u64 *part_off, const u32 *part_stride, u32 *counts_out, u32 cstride, u64 *failure)
{
    const u32 cap = split_capacity(hstride);
    if (!k || !cap) throw std::invalid_argument("k < 1, or no instance for this hstride");
    std::fill(counts_out, counts_out + (size_t)k * cstride, 0u);
    const u32 T = split_threads(cap), per = cap / T, waves = T / 64;
    std::vector<u64> key(cap);
    std::vector<u32> sum(T), incl(T), wave_total(waves);
    for (u32 rank = 0; rank < n_occ; rank++) {
        const u32 slot = occ[rank], cnt = counts[slot], nf = found[rank];
        const u64 *list = hits + (size_t)rank * hstride;
        const u32 *ml = mult + (size_t)rank * hstride;
        for (u32 tid = 0; tid < T; tid++)
            for (u32 i = tid; i < cap; i += T) key[i] = i < hstride ? split_load(list, ml, i, nf, cnt) : SPLIT_SENTINEL;
        for (u32 size = 2; size <= cap; size <<= 1)
            for (u32 j = size >> 1; j; j >>= 1)
                for (u32 tid = 0; tid < T; tid++)
                    for (u32 i = tid; i < cap / 2; i += T) {
                        u32 lo, hi;
                        split_pair(i, j, lo, hi);
                        split_exchange(key[lo], key[hi], split_ascending(lo, size));
                    }
        for (u32 tid = 0; tid < T; tid++) {
            sum[tid] = 0;
            for (u32 e = 0; e < per; e++) sum[tid] = split_combine(sum[tid], split_key_mult(key[tid * per + e]));
        }
        incl = sum;                                             // the wave's scan, step by step over all lanes at once
        for (u32 d = 1; d < 64; d <<= 1) {
            const std::vector<u32> prev = incl;
            for (u32 tid = 0; tid < T; tid++)
                if ((tid & 63) >= d) incl[tid] = split_combine(prev[tid], prev[tid - d]);
        }
        for (u32 w = 0; w < waves; w++) wave_total[w] = incl[w * 64 + 63];
        u32 total = 0;
        for (u32 w = 0; w < waves; w++) total = split_combine(total, wave_total[w]);
        if (!split_bin_ok(nf, cnt, total)) {
            *failure = std::min(*failure, split_failure(slot, nf, cnt, total));
            continue;
        }
        for (u32 tid = 0; tid < T; tid++) {
            u32 before = 0;
            for (u32 w = 0; w < (tid >> 6); w++) before = split_combine(before, wave_total[w]);
            u32 pos = split_combine(before, incl[tid] - sum[tid]);
            for (u32 e = 0; e < per; e++) {
                const u64 kx = key[tid * per + e];
                const u32 m = split_key_mult(kx);
                split_write(out, part_off, part_stride, slot, cnt, k, pos, m, split_key_value(kx));
                pos = split_combine(pos, m);
            }
        }
        for (u32 p = 0; p < k; p++) counts_out[(size_t)p * cstride + slot] = split_cut(cnt, k, p + 1) - split_cut(cnt, k, p);
    }
}

// ---- host rules
// the smallest k >= 1 with ceil(max_count / k) < limit: the placement rule's strict bound, so that every part takes insertions and can
// be exported
inline u32 split_parts(u32 max_count, u32 limit)
{
    if (!limit || (limit < 2 && max_count)) throw std::invalid_argument("split_parts: no bin of " + std::to_string(max_count) + " items can be cut below " + std::to_string(limit));
    if (max_count < limit) return 1;
    return (max_count + limit - 2) / (limit - 1);                 // ceil(max_count / k) <= limit - 1  <=>  k >= max_count / (limit - 1)
}

// what the host knows of a split without any root: per part its counts [n] (LOOKUP_NONE kept) and its degree
struct SplitShape {
    std::vector<u32> counts;                                      // [k][n]
    std::vector<u32> degree;                                      // [k]
};
inline SplitShape split_shape(const u32 *counts, size_t n, u32 k, u32 none)
{
    SplitShape s;
    s.counts.resize((size_t)k * n);
    s.degree.assign(k, 0);
    for (u32 p = 0; p < k; p++)
        for (size_t i = 0; i < n; i++) {
            const u32 c = counts[i];
            const u32 part = c == none ? none : split_cut(c, k, p + 1) - split_cut(c, k, p);
            s.counts[(size_t)p * n + i] = part;
            if (c != none) s.degree[p] = std::max(s.degree[p], part);
        }
    return s;
}

}  // namespace apsu_he
