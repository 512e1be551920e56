// Launch entry points of kernels_bucket.hip: the database side's grouping by location on the device, and the gather of the entries.
// Rules: bucket_plan.h.
#pragma once
#include <hip/hip_runtime.h>
#include "bucket_plan.h"

namespace apsu_he {

// the workspace of one launch_bucket_sort, in words of each type, for `count` items under H functions and tiles of `tile` keys
struct BucketSizes {
    u64 entries;                                          // count * H: the keys' room
    u64 key_tiles, tiles;                                 // tiles of items (key generation), tiles of keys (the passes)
    u32 digits;                                           // counters per wave: 1 << the widest digit
    size_t keys, tile_cnt, tile_base, hist, wave_cnt, scanned;
};
inline BucketSizes bucket_sizes(size_t count, u32 H, u32 T, u32 tile)
{
    BucketSizes s{};
    const BucketDigits d = bucket_digit_plan(T);
    s.entries = (u64)count * H;
    s.key_tiles = bucket_tiles(count, tile);
    s.tiles = bucket_tiles(s.entries, tile);
    s.digits = d.passes ? 1u << d.width[0] : 1;
    s.keys = s.entries;
    s.tile_cnt = s.tile_base = s.key_tiles;
    s.hist = s.scanned = (size_t)s.tiles * s.digits;
    s.wave_cnt = s.hist * BUCKET_WAVES;
    return s;
}
struct BucketWork {
    u64 *keys[2];                                         // [entries] each: the passes go from one to the other
    u32 *tile_cnt; u64 *tile_base;                        // [key_tiles]
    u32 *hist, *wave_cnt; u64 *scanned;                   // [digits][tiles], [tiles][waves][digits], [digits][tiles]
    u64 *total;                                           // one word: the surviving entries
};

// locs [count][H] (device) -> offsets [T + 1] (u64), order [*total] (u32; `entries` words of room, the words past *total are not
// written), w.total -- all on the device; nothing is waited for.  contract: 1 <= count < 2^32 - 1, 1 <= H <= BUCKET_MAX_FUNCS, T >= 1,
// every location < T (a larger one is sorted by its low bits: wrong words, no access out of bounds), bucket_tile_ok(tile), the
// buffers of bucket_sizes.  Launches: 3 for the keys, 3 per pass of bucket_digit_plan(T), 2 for offsets and order.
// -> the sorted keys (one of w.keys).
const u64 *launch_bucket_sort(const u32 *locs, size_t count, u32 H, u32 T, u32 tile, const BucketWork &w, u64 *offsets, u32 *order, hipStream_t st);

// The launches of launch_bucket_sort one by one, each with the grid and block it has there (the sort calls these; so do the steps of
// engine_bucket_steps.cpp).  All pointers are device memory, nothing is waited for.  std::logic_error outside the contracts.
// tile_cnt[t] = the surviving entries of items t tile .. of locs [count][H], t < bucket_tiles(count, tile).  contract: 1 <= count <
// 2^32 - 1, 1 <= H <= BUCKET_MAX_FUNCS, bucket_tile_ok(tile) -- for the keys as well:
void launch_bucket_count(const u32 *locs, size_t count, u32 H, u32 tile, u32 *tile_cnt, hipStream_t st);
// keys[tile_base[t] ..] = the keys of tile t's surviving entries in (i, h) order; no other word of keys is written
void launch_bucket_keys(const u32 *locs, size_t count, u32 H, u32 tile, const u64 *tile_base, u64 *keys, hipStream_t st);
// out[k] = in[0] + .. + in[k - 1] for k < n, *sum = the sum of all n (sum may be null); one workgroup, n = 0 writes *sum alone
void launch_bucket_scan(const u32 *in, u64 n, u64 *out, u64 *sum, hipStream_t st);
// one pass over keys [tiles * tile] of which the first *total count: hist [1 << width][tiles], wave_cnt [tiles][BUCKET_WAVES][1 << width]
// (every word written, zeros for a tile beyond *total); the scatter writes out[scanned[d][t] + ..] for the keys below *total alone.
// contract: 1 <= tiles < 2^31, bucket_tile_ok(tile), 1 <= width <= BUCKET_DIGIT_BITS, 32 <= shift, shift + width <= 64, *total <= tiles * tile
void launch_bucket_hist(const u64 *keys, const u64 *total, u64 tiles, u32 tile, u32 shift, u32 width, u32 *hist, u32 *wave_cnt, hipStream_t st);
void launch_bucket_scatter(const u64 *keys, const u64 *total, u64 tiles, u32 tile, u32 shift, u32 width, const u64 *scanned, const u32 *wave_cnt, u64 *out,
                           hipStream_t st);
// offsets[l] = the first of the *total ascending keys that is >= l << 32, l <= T (T >= 1); order[k] = the low half of keys[k], k < *total
// (`room` >= *total words of order sizes the grid; 0: nothing is launched)
void launch_bucket_offsets(const u64 *keys, const u64 *total, u32 T, u64 *offsets, hipStream_t st);
void launch_bucket_order(const u64 *keys, const u64 *total, u64 room, u32 *order, hipStream_t st);

// entries[k] = items[order[k]] for k < *total: one 16-byte load and one 16-byte store per lane.  items and entries 16-byte aligned.
void launch_entries_gather(const unsigned char *items, const u32 *order, const u64 *total, u64 room, unsigned char *entries, hipStream_t st);

} // namespace apsu_he
