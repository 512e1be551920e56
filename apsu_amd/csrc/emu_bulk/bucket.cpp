// CPU emulation of the database side's grouping on the device (bucket_plan.h; kernels_bucket.hip): the digit plan, the tile geometry,
// the wave-rank lane body, and the whole sort with every launch as explicit loops over its tiles, waves and lanes.  In
// libapsu_he_hostemu_bulk.so like the build that follows it on the route (bulk.cpp, which says why that library is apart); refusals
// leave their text in emu_bulk_last_error.  Only tests load it (tests/test_bucket_plan_cpu.py); it is not a fallback path.
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "../emu/emu_common.h"
#include "bucket_plan.h"

using namespace apsu_he;

namespace {

// __ballot over the 64 lanes of a wave
template <class Pred> u64 ballot(Pred pred)
{
    u64 m = 0;
    for (u32 lane = 0; lane < BUCKET_WAVE; lane++) if (pred(lane)) m |= (u64)1 << lane;
    return m;
}

// bucket_round of kernels_bucket.hip for all lanes of a wave at once: digit, rank and peers per lane
void wave_round(const u64 *key, u64 valid, u32 shift, u32 width, u32 *digit, u32 *rank, u32 *peers)
{
    for (u32 lane = 0; lane < BUCKET_WAVE; lane++) digit[lane] = bucket_digit(key[lane], shift, width);
    u64 bal[BUCKET_DIGIT_BITS];
    for (u32 bit = 0; bit < width; bit++) bal[bit] = ballot([&](u32 l) { return (digit[l] >> bit) & 1; });
    for (u32 lane = 0; lane < BUCKET_WAVE; lane++) {
        u64 mask = valid;
        for (u32 bit = 0; bit < width; bit++) mask = bucket_match(mask, bal[bit], (digit[lane] >> bit) & 1);
        rank[lane] = bucket_rank(mask, lane);
        peers[lane] = bucket_peers(mask);
    }
}

// k_bucket_scan
void scan(const std::vector<u32> &in, std::vector<u64> &out, u64 *sum)
{
    u64 run = 0;
    out.resize(in.size());
    for (size_t k = 0; k < in.size(); k++) { out[k] = run; run += in[k]; }
    if (sum) *sum = run;
}

} // namespace

extern "C" {

// out[10] = bits, passes, width[4], shift[4]
int emu_bucket_digit_plan(uint32_t T, uint32_t *out)
{
    const BucketDigits d = bucket_digit_plan(T);
    out[0] = d.bits; out[1] = d.passes;
    for (u32 p = 0; p < BUCKET_MAX_PASSES; p++) { out[2 + p] = d.width[p]; out[6 + p] = d.shift[p]; }
    return 0;
}

// out[4 + 2 waves] = tiles, the last tile's keys, the tile's least size and step, then [begin, end) of every wave's run in the last tile.
// -> the waves, or -1 for a tile size outside the rule
int emu_bucket_geometry(uint64_t entries, uint32_t tile, uint64_t *out)
{
    return guarded([&]() -> int {
        if (!bucket_tile_ok(tile)) throw std::invalid_argument("tile_entries outside the rule");
        const u64 tiles = bucket_tiles(entries, tile);
        const u32 len = tiles ? bucket_tile_len(entries, tile, tiles - 1) : 0;
        out[0] = tiles; out[1] = len; out[2] = BUCKET_TILE_MIN; out[3] = BUCKET_TILE_STEP;
        if (bucket_tile_len(entries, tile, tiles)) throw std::logic_error("a tile beyond the last holds keys");
        for (u32 w = 0; w < BUCKET_WAVES; w++) {
            u32 b, e;
            bucket_wave_run(tile, len, w, &b, &e);
            out[4 + 2 * w] = b; out[5 + 2 * w] = e;
        }
        return (int)BUCKET_WAVES;
    });
}

// the wave-rank lane body: digit[64] of `width` bits, valid = the lanes that hold a key -> rank[64], peers[64] (of the valid lanes)
int emu_bucket_wave_rank(const uint32_t *digit, uint64_t valid, uint32_t width, uint32_t *rank, uint32_t *peers)
{
    return guarded([&]() -> int {
        if (width > BUCKET_DIGIT_BITS) throw std::invalid_argument("a digit has at most 8 bits");
        u64 key[BUCKET_WAVE];
        u32 d[BUCKET_WAVE];
        for (u32 lane = 0; lane < BUCKET_WAVE; lane++) key[lane] = (u64)digit[lane] << 32;
        wave_round(key, valid, 32, width, d, rank, peers);
        return 0;
    });
}

// launch_bucket_sort, launch by launch: locs [count][H] -> offsets [T + 1], order [*total] (count * H words of room; the words past
// *total are not written).  -> the passes run, or -1: the hook's refusals (apsu_he_debug_bucket_locs), nothing written.
int emu_bucket_sort(const uint32_t *locs, uint64_t count, uint32_t H, uint32_t T, uint32_t tile, uint64_t *offsets, uint32_t *order, uint64_t *total)
{
    return guarded([&]() -> int {
        if (!H || H > BUCKET_MAX_FUNCS || !T) throw std::invalid_argument("1 <= H <= 8 and T >= 1");
        if (count >= 0xFFFFFFFFull) throw std::invalid_argument("more items than a 32-bit index names");
        if (!tile) tile = BUCKET_TILE_DEFAULT;
        if (!bucket_tile_ok(tile)) throw std::invalid_argument("tile_entries outside the rule");
        for (u64 k = 0; k < count * H; k++) if (locs[k] >= T) throw std::invalid_argument("location " + std::to_string(k) + " is outside the table");
        for (u64 l = 0; l <= T; l++) offsets[l] = 0;
        *total = 0;
        if (!count) return 0;
        const BucketDigits plan = bucket_digit_plan(T);
        const u64 room = count * H, key_tiles = bucket_tiles(count, tile), tiles = bucket_tiles(room, tile);
        // k_bucket_count, k_bucket_scan, k_bucket_keys: tiles of items, 256 a step
        std::vector<u32> tile_cnt(key_tiles, 0);
        for (u64 t = 0; t < key_tiles; t++)
            for (u64 i = t * tile; i < std::min<u64>(t * tile + tile, count); i++) tile_cnt[t] += bucket_item_count(locs + i * H, H);
        std::vector<u64> tile_base;
        u64 n = 0;
        scan(tile_cnt, tile_base, &n);
        std::vector<u64> keys[2] = { std::vector<u64>(room, ~(u64)0), std::vector<u64>(room, ~(u64)0) };
        for (u64 t = 0; t < key_tiles; t++) {
            const u64 end = std::min<u64>(t * tile + tile, count);
            u64 base = tile_base[t];
            for (u64 i0 = t * tile; i0 < end; i0 += BUCKET_T) {
                u32 c[BUCKET_T], all = 0;
                for (u32 tid = 0; tid < (u32)BUCKET_T; tid++) c[tid] = i0 + tid < end ? bucket_item_count(locs + (i0 + tid) * H, H) : 0;
                for (u32 tid = 0; tid < (u32)BUCKET_T; tid++) {
                    u64 pos = base + all;                              // (the lanes before this one, whatever their wave)
                    all += c[tid];
                    if (i0 + tid >= end) continue;
                    const u32 *li = locs + (i0 + tid) * H;
                    for (u32 h = 0; h < H; h++)
                        if (bucket_first_use(li, h)) keys[0].at(pos++) = bucket_key(li[h], (u32)(i0 + tid));
                }
                base += all;
            }
        }
        u32 at = 0;
        for (u32 p = 0; p < plan.passes; p++, at ^= 1) {
            const u32 shift = plan.shift[p], width = plan.width[p], D = 1u << width;
            const std::vector<u64> &src = keys[at];
            std::vector<u64> &dst = keys[at ^ 1];
            // k_bucket_hist
            std::vector<u32> hist((size_t)tiles * D, 0), wave_cnt((size_t)tiles * BUCKET_WAVES * D, 0);
            for (u64 t = 0; t < tiles; t++) {
                const u32 len = bucket_tile_len(n, tile, t);
                for (u32 w = 0; w < BUCKET_WAVES; w++) {
                    u32 b, e;
                    bucket_wave_run(tile, len, w, &b, &e);
                    u32 *mine = wave_cnt.data() + (t * BUCKET_WAVES + w) * D;
                    for (u32 r = b; r < e; r += BUCKET_WAVE) {
                        u64 key[BUCKET_WAVE];
                        u32 digit[BUCKET_WAVE], rank[BUCKET_WAVE], peers[BUCKET_WAVE];
                        const u64 valid = ballot([&](u32 l) { return r + l < e; });
                        for (u32 lane = 0; lane < BUCKET_WAVE; lane++) key[lane] = r + lane < e ? src.at(t * tile + r + lane) : 0;
                        wave_round(key, valid, shift, width, digit, rank, peers);
                        for (u32 lane = 0; lane < BUCKET_WAVE; lane++)
                            if (r + lane < e && rank[lane] == 0) mine[digit[lane]] += peers[lane];
                    }
                    for (u32 d = 0; d < D; d++) hist[(size_t)d * tiles + t] += mine[d];
                }
            }
            // k_bucket_scan over (digit major, tile minor)
            std::vector<u64> scanned;
            scan(hist, scanned, nullptr);
            // k_bucket_scatter
            for (u64 t = 0; t < tiles; t++) {
                const u32 len = bucket_tile_len(n, tile, t);
                if (!len) continue;
                std::vector<u64> base((size_t)BUCKET_WAVES * D);
                for (u32 d = 0; d < D; d++) {
                    u64 run = scanned[(size_t)d * tiles + t];
                    for (u32 w = 0; w < BUCKET_WAVES; w++) { base[(size_t)w * D + d] = run; run += wave_cnt[(t * BUCKET_WAVES + w) * D + d]; }
                }
                for (u32 w = 0; w < BUCKET_WAVES; w++) {
                    u32 b, e;
                    bucket_wave_run(tile, len, w, &b, &e);
                    u64 *mine = base.data() + (size_t)w * D;
                    for (u32 r = b; r < e; r += BUCKET_WAVE) {
                        u64 key[BUCKET_WAVE], pos[BUCKET_WAVE];
                        u32 digit[BUCKET_WAVE], rank[BUCKET_WAVE], peers[BUCKET_WAVE];
                        const u64 valid = ballot([&](u32 l) { return r + l < e; });
                        for (u32 lane = 0; lane < BUCKET_WAVE; lane++) key[lane] = r + lane < e ? src.at(t * tile + r + lane) : 0;
                        wave_round(key, valid, shift, width, digit, rank, peers);
                        for (u32 lane = 0; lane < BUCKET_WAVE; lane++) pos[lane] = r + lane < e ? mine[digit[lane]] : 0;      // every lane reads ...
                        for (u32 lane = 0; lane < BUCKET_WAVE; lane++) {                                                    // ... before one writes
                            if (r + lane >= e) continue;
                            u64 &slot = dst.at(pos[lane] + rank[lane]);
                            if (pos[lane] + rank[lane] >= n || slot != ~(u64)0) throw std::logic_error("a place was taken twice, or lies beyond the keys");
                            slot = key[lane];
                            if (rank[lane] + 1 == peers[lane]) mine[digit[lane]] = pos[lane] + peers[lane];
                        }
                    }
                }
            }
            std::fill(keys[at].begin(), keys[at].end(), ~(u64)0);         // (the next pass's check that every place is written once)
        }
        // k_bucket_offsets, k_bucket_order
        const u64 *sorted = keys[at].data();
        for (u64 l = 0; l <= T; l++) offsets[l] = bucket_lower_bound(sorted, n, l << 32);
        for (u64 k = 0; k < n; k++) order[k] = bucket_key_item(sorted[k]);
        *total = n;
        return (int)plan.passes;
    });
}

} // extern "C"
