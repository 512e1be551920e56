// The database side's grouping on the device (Engine::items_bucket_device; kernels_bucket.hip): the rules as pure functions.  No HIP in
// here; the CPU tier steps them tile by tile, wave by wave and lane by lane (emu_bulk/bucket.cpp: emu_bucket_sort in
// libapsu_he_hostemu_bulk.so; tests/test_bucket_plan_cpu.py).  The specification stays cuckoo_bucket (cuckoo.h).
//
// The output of cuckoo_bucket is the sequence of the surviving pairs (loc, i) -- entry (i, h) survives iff no g < h has
// locs[i][g] == locs[i][h] -- in ascending (loc, i) order: order = the i, offsets[l] = the pairs with loc < l.  The pairs are made in
// (i, h) order, which is ascending in i, so a STABLE sort by loc alone gives that sequence:
//   keys     key = loc << 32 | i of every surviving entry, compacted in (i, h) order (bucket_first_use; a count, a scan, a write).
//   passes   a least-significant-digit radix sort on the ceil(log2 T) bits of loc, in digits of at most 8 bits (bucket_digit_plan).
//            Per pass: a histogram per tile and per wave of the tile (k_bucket_hist), one exclusive scan over (digit major, tile
//            minor) (k_bucket_scan), a stable scatter (k_bucket_scatter).  A tile is `tile` consecutive keys, a wave owns a
//            contiguous quarter of it (bucket_wave_run) and walks it 64 keys at a time; a lane's rank among the lanes of its wave with
//            the same digit comes from ballots, digit bit by digit bit (bucket_match, bucket_rank); the waves of a tile are ordered
//            through the [waves][digits] counts the histogram kernel left.
//   offsets  offsets[l] = the first sorted key >= l << 32, by bisection (bucket_lower_bound); order = the keys' low halves.
// No rank comes from an atomic's return value and no workgroup waits for another: every pass over the data is a launch of its own.
#pragma once
#include <stddef.h>
#include "modmath.h"

namespace apsu_he {

constexpr int BUCKET_T = 256;                             // lanes per workgroup of the tile kernels
constexpr u32 BUCKET_WAVE = 64;
constexpr u32 BUCKET_WAVES = BUCKET_T / BUCKET_WAVE;
constexpr u32 BUCKET_DIGIT_BITS = 8;                      // the widest digit: 256 counters per wave in LDS
constexpr u32 BUCKET_MAX_PASSES = 4;                      // 32 bits of location
constexpr u32 BUCKET_MAX_FUNCS = 8;                       // hash_func_count's bound (cuckoo.h: CUCKOO_MAX_FUNCS)
// keys per tile: every wave takes whole rounds of 64 lanes, so the least tile is one round per wave and tiles come in steps of that
constexpr u32 BUCKET_TILE_MIN = BUCKET_T, BUCKET_TILE_STEP = BUCKET_T, BUCKET_TILE_MAX = 1u << 20;
constexpr u32 BUCKET_TILE_DEFAULT = 8192;                 // (profiles/r28_bucket.txt)
constexpr int BUCKET_SCAN_T = 1024;                       // the scan's one workgroup ...
constexpr u32 BUCKET_SCAN_PER_LANE = 8;                   // ... takes this many consecutive words per lane and step

// ---- the digit plan: T -> passes and bits per pass, least significant digit first
struct BucketDigits {
    u32 bits;                                             // ceil(log2 T): what tells two locations below T apart
    u32 passes;                                           // ceil(bits / 8); T = 1: none, the keys are sorted as made
    u32 width[BUCKET_MAX_PASSES], shift[BUCKET_MAX_PASSES];   // pass p sorts on bits [shift, shift + width) of the key, shift >= 32
};
HD BucketDigits bucket_digit_plan(u32 T)
{
    BucketDigits d{};
    while (d.bits < 32 && ((u64)1 << d.bits) < T) d.bits++;
    d.passes = (d.bits + BUCKET_DIGIT_BITS - 1) / BUCKET_DIGIT_BITS;
    u32 at = 32;
    for (u32 p = 0; p < d.passes; p++) {                  // as even as whole bits allow, the wider digits first
        d.width[p] = d.bits / d.passes + (p < d.bits % d.passes ? 1 : 0);
        d.shift[p] = at;
        at += d.width[p];
    }
    return d;
}
HD u32 bucket_digit(u64 key, u32 shift, u32 width) { return (u32)(key >> shift) & ((1u << width) - 1); }

// ---- the keys
HD u64 bucket_key(u32 loc, u32 i) { return ((u64)loc << 32) | i; }
HD u32 bucket_key_item(u64 key) { return (u32)key; }
// cuckoo_bucket's first_use: entry (i, h) counts unless an earlier function of the item gave the same location
HD bool bucket_first_use(const u32 *li, u32 h)
{
    for (u32 g = 0; g < h; g++) if (li[g] == li[h]) return false;
    return true;
}
// the surviving entries of an item (1 .. H for H >= 1)
HD u32 bucket_item_count(const u32 *li, u32 H)
{
    u32 c = 0;
    for (u32 h = 0; h < H; h++) c += bucket_first_use(li, h) ? 1 : 0;
    return c;
}

// ---- the tile geometry
HD bool bucket_tile_ok(u32 tile) { return tile >= BUCKET_TILE_MIN && tile <= BUCKET_TILE_MAX && tile % BUCKET_TILE_STEP == 0; }
HD u64 bucket_tiles(u64 entries, u32 tile) { return (entries + tile - 1) / tile; }
// keys of tile t (the last one may be ragged; a tile at or beyond the end has none)
HD u32 bucket_tile_len(u64 entries, u32 tile, u64 t)
{
    const u64 first = t * tile;
    return first >= entries ? 0 : (entries - first < tile ? (u32)(entries - first) : tile);
}
// wave w of a tile of `len` keys owns keys [*begin, *end) of the tile: a contiguous run of tile / BUCKET_WAVES, cut at len
HD void bucket_wave_run(u32 tile, u32 len, u32 w, u32 *begin, u32 *end)
{
    const u32 run = tile / BUCKET_WAVES;
    const u32 b = w * run, e = b + run;
    *begin = b < len ? b : len;
    *end = e < len ? e : len;
}

// ---- the wave-rank lane body.  `mask` starts as the ballot of the lanes that hold a key; for every bit of the digit, `ballot` = the
// lanes whose digit has that bit set: afterwards mask = the lanes of the wave whose digit equals this lane's.
HD u64 bucket_match(u64 mask, u64 ballot, bool bit_set) { return mask & (bit_set ? ballot : ~ballot); }
HD u32 bucket_rank(u64 mask, u32 lane) { return (u32)__builtin_popcountll(mask & (((u64)1 << lane) - 1)); }      // peers in lower lanes
HD u32 bucket_peers(u64 mask) { return (u32)__builtin_popcountll(mask); }

// ---- offsets: the first of `total` ascending keys that is >= bound
template <class Keys> HD u64 bucket_lower_bound(const Keys &keys, u64 total, u64 bound)
{
    u64 lo = 0, hi = total;
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if (keys[mid] < bound) lo = mid + 1; else hi = mid;
    }
    return lo;
}

} // namespace apsu_he
