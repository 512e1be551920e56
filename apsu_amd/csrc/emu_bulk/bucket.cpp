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

// ---- the kernels of kernels_bucket.hip one by one, on host arrays with the launchers' arguments (launch_bucket.h).  emu_bucket_sort
// below calls them in launch_bucket_sort's order; the entry points behind it give each of them alone to the tests.
// k_bucket_count: a workgroup per tile of items
void count(const u32 *locs, u64 n_items, u32 H, u32 tile, u32 *tile_cnt)
{
    for (u64 t = 0; t < bucket_tiles(n_items, tile); t++) {
        u32 c = 0;
        for (u64 i = t * tile; i < std::min<u64>(t * tile + tile, n_items); i++) c += bucket_item_count(locs + i * H, H);
        tile_cnt[t] = c;
    }
}

// k_bucket_keys: 256 items a step; a lane's place = the tile's base + the entries of the lanes before it
void keys_of(const u32 *locs, u64 n_items, u32 H, u32 tile, const u64 *tile_base, u64 *keys)
{
    for (u64 t = 0; t < bucket_tiles(n_items, tile); t++) {
        const u64 end = std::min<u64>(t * tile + tile, n_items);
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
                    if (bucket_first_use(li, h)) keys[pos++] = bucket_key(li[h], (u32)(i0 + tid));
            }
            base += all;
        }
    }
}

// k_bucket_scan as its one workgroup steps it: BUCKET_SCAN_T lanes take BUCKET_SCAN_PER_LANE consecutive words each, the waves'
// inclusive sums go through wtot[step & 1], a 64-bit carry goes from step to step.  (The lanes run one after the other here: what the
// double buffer guards, a wave of step s + 1 writing while another still reads step s, cannot show.)
void scan(const u32 *in, u64 n, u64 *out, u64 *sum)
{
    constexpr u32 LANES = BUCKET_SCAN_T, WAVES = LANES / BUCKET_WAVE, PER = BUCKET_SCAN_PER_LANE;
    u64 wtot[2][WAVES];
    u64 carry = 0;
    u32 step = 0;
    std::vector<u32> v((size_t)LANES * PER);
    std::vector<u64> s(LANES), inc(LANES);
    for (u64 c0 = 0; c0 < n; c0 += (u64)LANES * PER, step++) {
        for (u32 tid = 0; tid < LANES; tid++) {
            const u64 first = c0 + (u64)tid * PER;
            s[tid] = 0;
            for (u32 j = 0; j < PER; j++) { v[tid * PER + j] = first + j < n ? in[first + j] : 0; s[tid] += v[tid * PER + j]; }
        }
        for (u32 w = 0; w < WAVES; w++) {                              // wave_inclusive, and the last lane's vote
            u64 run = 0;
            for (u32 lane = 0; lane < BUCKET_WAVE; lane++) { run += s[w * BUCKET_WAVE + lane]; inc[w * BUCKET_WAVE + lane] = run; }
            wtot[step & 1][w] = run;
        }
        u64 all = 0;
        for (u32 w = 0; w < WAVES; w++) all += wtot[step & 1][w];
        for (u32 tid = 0; tid < LANES; tid++) {
            const u32 w = tid / BUCKET_WAVE;
            const u64 first = c0 + (u64)tid * PER;
            u64 before = 0;
            for (u32 ww = 0; ww < w; ww++) before += wtot[step & 1][ww];
            u64 run = carry + before + inc[tid] - s[tid];
            for (u32 j = 0; j < PER; j++) {
                if (first + j < n) out[first + j] = run;
                run += v[tid * PER + j];
            }
        }
        carry += all;
    }
    if (sum) *sum = carry;
}

// k_bucket_hist: every tile of the grid writes its counters
void hist_of(const u64 *keys, u64 total, u64 tiles, u32 tile, u32 shift, u32 width, u32 *hist, u32 *wave_cnt)
{
    const u32 D = 1u << width;
    for (u64 t = 0; t < tiles; t++) {
        const u32 len = bucket_tile_len(total, tile, t);
        for (u32 d = 0; d < D; d++) hist[(size_t)d * tiles + t] = 0;
        for (u32 w = 0; w < BUCKET_WAVES; w++) {
            u32 b, e;
            bucket_wave_run(tile, len, w, &b, &e);
            u32 *mine = wave_cnt + (t * BUCKET_WAVES + w) * D;
            for (u32 d = 0; d < D; d++) mine[d] = 0;
            for (u32 r = b; r < e; r += BUCKET_WAVE) {
                u64 key[BUCKET_WAVE];
                u32 digit[BUCKET_WAVE], rank[BUCKET_WAVE], peers[BUCKET_WAVE];
                const u64 valid = ballot([&](u32 l) { return r + l < e; });
                for (u32 lane = 0; lane < BUCKET_WAVE; lane++) key[lane] = r + lane < e ? keys[t * tile + r + lane] : 0;
                wave_round(key, valid, shift, width, digit, rank, peers);
                for (u32 lane = 0; lane < BUCKET_WAVE; lane++)
                    if (r + lane < e && rank[lane] == 0) mine[digit[lane]] += peers[lane];
            }
            for (u32 d = 0; d < D; d++) hist[(size_t)d * tiles + t] += mine[d];
        }
    }
}

// k_bucket_scatter.  `room` = the words of out; strict (the whole sort's own check): a place is below total and holds ~0 until its key comes
void scatter(const u64 *keys, u64 total, u64 tiles, u32 tile, u32 shift, u32 width, const u64 *scanned, const u32 *wave_cnt, u64 *out, u64 room, bool strict)
{
    const u32 D = 1u << width;
    for (u64 t = 0; t < tiles; t++) {
        const u32 len = bucket_tile_len(total, tile, t);
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
                for (u32 lane = 0; lane < BUCKET_WAVE; lane++) key[lane] = r + lane < e ? keys[t * tile + r + lane] : 0;
                wave_round(key, valid, shift, width, digit, rank, peers);
                for (u32 lane = 0; lane < BUCKET_WAVE; lane++) pos[lane] = r + lane < e ? mine[digit[lane]] : 0;      // every lane reads ...
                for (u32 lane = 0; lane < BUCKET_WAVE; lane++) {                                                    // ... before one writes
                    if (r + lane >= e) continue;
                    const u64 at = pos[lane] + rank[lane];
                    if (at >= room) throw std::logic_error("a place lies beyond the room");
                    if (strict && (at >= total || out[at] != ~(u64)0)) throw std::logic_error("a place was taken twice, or lies beyond the keys");
                    out[at] = key[lane];
                    if (rank[lane] + 1 == peers[lane]) mine[digit[lane]] = pos[lane] + peers[lane];
                }
            }
        }
    }
}

// k_bucket_offsets, k_bucket_order, k_entries_gather
void offsets_of(const u64 *keys, u64 total, u32 T, u64 *offsets) { for (u64 l = 0; l <= T; l++) offsets[l] = bucket_lower_bound(keys, total, l << 32); }
void order_of(const u64 *keys, u64 total, u32 *order) { for (u64 k = 0; k < total; k++) order[k] = bucket_key_item(keys[k]); }

void geometry_ok(u32 tile, u32 shift, u32 width)
{
    if (!bucket_tile_ok(tile)) throw std::invalid_argument("tile_entries outside the rule");
    if (!width || width > BUCKET_DIGIT_BITS || shift < 32 || shift + width > 64) throw std::invalid_argument("1 <= width <= 8, 32 <= shift, shift + width <= 64");
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
int emu_bucket_sort(const uint32_t *locs, uint64_t count_items, uint32_t H, uint32_t T, uint32_t tile, uint64_t *offsets, uint32_t *order, uint64_t *total)
{
    return guarded([&]() -> int {
        if (!H || H > BUCKET_MAX_FUNCS || !T) throw std::invalid_argument("1 <= H <= 8 and T >= 1");
        if (count_items >= 0xFFFFFFFFull) throw std::invalid_argument("more items than a 32-bit index names");
        if (!tile) tile = BUCKET_TILE_DEFAULT;
        if (!bucket_tile_ok(tile)) throw std::invalid_argument("tile_entries outside the rule");
        for (u64 k = 0; k < count_items * H; k++) if (locs[k] >= T) throw std::invalid_argument("location " + std::to_string(k) + " is outside the table");
        for (u64 l = 0; l <= T; l++) offsets[l] = 0;
        *total = 0;
        if (!count_items) return 0;
        const BucketDigits plan = bucket_digit_plan(T);
        const u64 room = count_items * H, key_tiles = bucket_tiles(count_items, tile), tiles = bucket_tiles(room, tile);
        // k_bucket_count, k_bucket_scan, k_bucket_keys: tiles of items, 256 a step
        std::vector<u32> tile_cnt(key_tiles, 0);
        count(locs, count_items, H, tile, tile_cnt.data());
        std::vector<u64> tile_base(key_tiles);
        u64 n = 0;
        scan(tile_cnt.data(), key_tiles, tile_base.data(), &n);
        std::vector<u64> keys[2] = { std::vector<u64>(room, ~(u64)0), std::vector<u64>(room, ~(u64)0) };
        for (u64 t = 0; t < key_tiles; t++) if (tile_base[t] + tile_cnt[t] > room) throw std::logic_error("a tile's keys lie beyond the room");
        keys_of(locs, count_items, H, tile, tile_base.data(), keys[0].data());
        u32 at = 0;
        for (u32 p = 0; p < plan.passes; p++, at ^= 1) {
            const u32 shift = plan.shift[p], width = plan.width[p], D = 1u << width;
            // k_bucket_hist, k_bucket_scan over (digit major, tile minor), k_bucket_scatter
            std::vector<u32> hist((size_t)tiles * D, 0), wave_cnt((size_t)tiles * BUCKET_WAVES * D, 0);
            hist_of(keys[at].data(), n, tiles, tile, shift, width, hist.data(), wave_cnt.data());
            std::vector<u64> scanned(hist.size());
            scan(hist.data(), hist.size(), scanned.data(), nullptr);
            scatter(keys[at].data(), n, tiles, tile, shift, width, scanned.data(), wave_cnt.data(), keys[at ^ 1].data(), room, true);
            std::fill(keys[at].begin(), keys[at].end(), ~(u64)0);         // (the next pass's check that every place is written once)
        }
        // k_bucket_offsets, k_bucket_order
        offsets_of(keys[at].data(), n, T, offsets);
        order_of(keys[at].data(), n, order);
        *total = n;
        return (int)plan.passes;
    });
}

// ---- every kernel alone, with its launcher's arguments on host arrays (the steps of engine_bucket_steps.cpp; tests/bucket_step_model.py).
// -> 0, or -1 with the reason in emu_bulk_last_error and nothing written: what the steps refuse.
int emu_bucket_count(const uint32_t *locs, uint64_t count_items, uint32_t H, uint32_t tile, uint32_t *tile_cnt)
{
    return guarded([&]() -> int {
        if (!H || H > BUCKET_MAX_FUNCS || !count_items) throw std::invalid_argument("1 <= H <= 8 and count >= 1");
        geometry_ok(tile, 32, 1);
        count(locs, count_items, H, tile, tile_cnt);
        return 0;
    });
}

int emu_bucket_keys(const uint32_t *locs, uint64_t count_items, uint32_t H, uint32_t tile, const uint64_t *tile_base, uint64_t *keys, uint64_t room)
{
    return guarded([&]() -> int {
        if (!H || H > BUCKET_MAX_FUNCS || !count_items) throw std::invalid_argument("1 <= H <= 8 and count >= 1");
        geometry_ok(tile, 32, 1);
        const u64 key_tiles = bucket_tiles(count_items, tile);
        std::vector<u32> cnt(key_tiles);
        count(locs, count_items, H, tile, cnt.data());
        for (u64 t = 0; t < key_tiles; t++) if (tile_base[t] > room || cnt[t] > room - tile_base[t]) throw std::invalid_argument("a tile's keys reach beyond the room");
        keys_of(locs, count_items, H, tile, tile_base, keys);
        return 0;
    });
}

int emu_bucket_scan(const uint32_t *in, uint64_t n, uint64_t *out, uint64_t *sum)
{
    return guarded([&]() -> int { scan(in, n, out, sum); return 0; });
}

int emu_bucket_hist(const uint64_t *keys, uint64_t total, uint64_t tiles, uint32_t tile, uint32_t shift, uint32_t width, uint32_t *hist, uint32_t *wave_cnt)
{
    return guarded([&]() -> int {
        geometry_ok(tile, shift, width);
        if (!tiles || total > tiles * tile) throw std::invalid_argument("a total above the keys given");
        hist_of(keys, total, tiles, tile, shift, width, hist, wave_cnt);
        return 0;
    });
}

// the places are checked against `room` on a copy first: a refusal writes nothing
int emu_bucket_scatter(const uint64_t *keys, uint64_t total, uint64_t tiles, uint32_t tile, uint32_t shift, uint32_t width, const uint64_t *scanned,
                       const uint32_t *wave_cnt, uint64_t *out, uint64_t room)
{
    return guarded([&]() -> int {
        geometry_ok(tile, shift, width);
        if (!tiles || total > tiles * tile) throw std::invalid_argument("a total above the keys given");
        std::vector<u64> trial(out, out + room);
        scatter(keys, total, tiles, tile, shift, width, scanned, wave_cnt, trial.data(), room, false);
        std::copy(trial.begin(), trial.end(), out);
        return 0;
    });
}

int emu_bucket_offsets(const uint64_t *keys, uint64_t total, uint32_t T, uint64_t *offsets)
{
    return guarded([&]() -> int {
        if (!T) throw std::invalid_argument("T >= 1");
        offsets_of(keys, total, T, offsets);
        return 0;
    });
}

int emu_bucket_order(const uint64_t *keys, uint64_t total, uint32_t *order)
{
    return guarded([&]() -> int { order_of(keys, total, order); return 0; });
}

// k_entries_gather: entries[k] = items[order[k]], 16 bytes each, k < total
int emu_entries_gather(const unsigned char *items, uint64_t count_items, const uint32_t *order, uint64_t total, unsigned char *entries)
{
    return guarded([&]() -> int {
        for (u64 k = 0; k < total; k++) if (order[k] >= count_items) throw std::invalid_argument("an order word names no item");
        for (u64 k = 0; k < total; k++) std::copy(items + (size_t)order[k] * 16, items + (size_t)order[k] * 16 + 16, entries + k * 16);
        return 0;
    });
}

} // extern "C"
