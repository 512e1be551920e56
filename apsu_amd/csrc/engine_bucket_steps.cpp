// One kernel of the database side's grouping at a time on caller-chosen words (Engine::debug_run_step from STEP_BUCKET_COUNT on;
// include/apsu_he.h).  As the other engine_*_steps.cpp do for their families: a step copies host arrays up, calls THE launcher that
// launch_bucket_sort calls for that kernel (launch_bucket.h), synchronises and copies back.  No chain level and no context constant is
// used.  A 32-bit array (locs, tile_cnt, hist, wave_cnt, order) travels as one 64-bit word per value and is narrowed here.  Every out[]
// is copied up first, so a word the kernel does not write comes back as it went.  Whatever a launcher's contract does not admit -- and
// every place a kernel would store beyond the caller's room, worked out here on the host -- is refused before anything is launched.
// For the tests; nothing on the database-building path calls it.
#include "engine_impl.h"
#include "launch_bucket.h"

#include <functional>
#include <list>
#include <string>

namespace apsu_he {

namespace {

[[noreturn]] void refuse(const std::string &why) { throw std::invalid_argument("debug_run_step: " + why); }
void need(bool ok, const char *why) { if (!ok) refuse(why); }

constexpr size_t WORDS_MAX = (size_t)1 << 26;                          // far above every test's arrays; keeps the products below small

} // namespace

void Engine::debug_run_bucket_step(const StepArgs &a)
{
    need(a.step >= STEP_BUCKET_COUNT && a.step <= STEP_ENTRIES_GATHER, "unknown step");
    const size_t terms = a.terms > 0 ? (size_t)a.terms : 0, polys = a.polys > 0 ? (size_t)a.polys : 0, batch = a.batch > 0 ? (size_t)a.batch : 0;
    auto in_is = [&](int i, size_t words, const char *what) { if (!a.in[i] || a.in_words[i] != words) refuse(std::string(what) + ": wrong size"); };
    auto out_is = [&](int i, size_t words, const char *what) { if (!a.out[i] || a.out_words[i] != words) refuse(std::string(what) + ": wrong size"); };
    auto fits32 = [&](const u64 *x, size_t words, const char *what) {
        u64 bad = 0;
        for (size_t i = 0; i < words; i++) bad |= x[i] >> 32;
        if (bad) refuse(std::string(what) + " holds a word that does not fit 32 bits");
    };
    for (int i = 0; i < 6; i++) need(!a.in[i] || a.in_words[i] <= WORDS_MAX, "an input array is too large");
    for (int i = 0; i < 2; i++) need(!a.out[i] || a.out_words[i] <= WORDS_MAX, "an output array is too large");

    // ---- the refusals, all in front of the arena: nothing below can refuse
    size_t count = 0, key_tiles = 0, n = 0, D = 0, T = 0, room = 0;
    u64 total = 0;
    const u32 tile = (u32)terms, H = (u32)polys, shift = a.e0 > 0 ? (u32)a.e0 : 0, width = a.n_ext > 0 ? (u32)a.n_ext : 0;
    switch (a.step) {
    case STEP_BUCKET_COUNT:
    case STEP_BUCKET_KEYS: {
        // polys = H, terms = tile; in[0] locs [count][H]; COUNT -> out[0] tile_cnt [key_tiles]; KEYS: in[1] tile_base [key_tiles] -> out[0] keys [room]
        need(terms <= 0xFFFFFFFFull && bucket_tile_ok(tile), "bucket_count / bucket_keys: a tile size (terms) outside the rule (bucket_tile_ok)");
        need(H >= 1 && H <= BUCKET_MAX_FUNCS, "bucket_count / bucket_keys: H (polys) outside 1 .. 8");
        need(a.in[0] && a.in_words[0] >= H && a.in_words[0] % H == 0, "bucket_count / bucket_keys: in[0] locs [count][H], count >= 1: wrong size");
        count = a.in_words[0] / H;
        key_tiles = (size_t)bucket_tiles(count, tile);
        fits32(a.in[0], a.in_words[0], "bucket_count / bucket_keys: in[0] (locs)");
        if (a.step == STEP_BUCKET_COUNT) { out_is(0, key_tiles, "bucket_count: out[0] tile_cnt [key_tiles]"); fits32(a.out[0], key_tiles, "bucket_count: out[0]"); break; }
        in_is(1, key_tiles, "bucket_keys: in[1] tile_base [key_tiles]");
        need(a.out[0] && a.out_words[0] >= 1, "bucket_keys: out[0] keys [room]: wrong size");
        room = a.out_words[0];
        std::vector<u32> li(H);
        for (size_t t = 0; t < key_tiles; t++) {
            u64 c = 0;
            for (size_t i = t * tile; i < std::min(t * tile + tile, count); i++) {
                for (u32 h = 0; h < H; h++) li[h] = (u32)a.in[0][i * H + h];
                c += bucket_item_count(li.data(), H);
            }
            need(a.in[1][t] <= room && c <= room - a.in[1][t], "bucket_keys: a tile's keys reach beyond the room of out[0]");
        }
    } break;
    case STEP_BUCKET_SCAN: {
        // in[0] [n] 32-bit values (null or empty: n = 0) -> out[0] [n + 1], the last word a guard; STORE: out[1] the sum, one word; else no out[1]
        n = a.in[0] ? a.in_words[0] : 0;
        if (n) fits32(a.in[0], n, "bucket_scan: in[0]");
        out_is(0, n + 1, "bucket_scan: out[0] [n + 1]");
        if (a.flags & STEP_STORE) out_is(1, 1, "bucket_scan: out[1] the sum, one word");
        else need(!a.out[1], "bucket_scan: out[1] without STORE (the launcher then gets no sum pointer)");
    } break;
    case STEP_BUCKET_HIST:
    case STEP_BUCKET_SCATTER: {
        // terms = tile, e0 = shift, n_ext = width, batch = the tiles of the grid; in[0] keys [batch * tile], in[1] total;
        // HIST -> out[0] hist [D][batch], out[1] wave_cnt [batch][waves][D]; SCATTER: in[2] scanned [D][batch], in[3] wave_cnt -> out[0] [room]
        need(terms <= 0xFFFFFFFFull && bucket_tile_ok(tile), "bucket_hist / bucket_scatter: a tile size (terms) outside the rule (bucket_tile_ok)");
        need(width >= 1 && width <= BUCKET_DIGIT_BITS, "bucket_hist / bucket_scatter: a width (n_ext) outside 1 .. 8");
        need(a.e0 >= 32 && shift + width <= 64, "bucket_hist / bucket_scatter: a shift (e0) below 32, or shift + width above 64");
        need(batch >= 1 && batch * (size_t)tile <= WORDS_MAX, "bucket_hist / bucket_scatter: tiles (batch) out of range");
        D = (size_t)1 << width;
        in_is(0, batch * tile, "bucket_hist / bucket_scatter: in[0] keys [batch * tile]");
        in_is(1, 1, "bucket_hist / bucket_scatter: in[1] total, one word");
        total = a.in[1][0];
        need(total <= batch * tile, "bucket_hist / bucket_scatter: a total above the keys given");
        if (a.step == STEP_BUCKET_HIST) {
            out_is(0, D * batch, "bucket_hist: out[0] hist [1 << width][batch]");
            out_is(1, batch * BUCKET_WAVES * D, "bucket_hist: out[1] wave_cnt [batch][4][1 << width]");
            fits32(a.out[0], a.out_words[0], "bucket_hist: out[0]");
            fits32(a.out[1], a.out_words[1], "bucket_hist: out[1]");
            break;
        }
        in_is(2, D * batch, "bucket_scatter: in[2] scanned [1 << width][batch]");
        in_is(3, batch * BUCKET_WAVES * D, "bucket_scatter: in[3] wave_cnt [batch][4][1 << width]");
        fits32(a.in[3], a.in_words[3], "bucket_scatter: in[3] (wave_cnt)");
        need(a.out[0] && a.out_words[0] >= 1, "bucket_scatter: out[0] [room]: wrong size");
        room = a.out_words[0];
        // the largest place of every (tile, wave, digit): the given scanned and wave_cnt, and the keys the wave's run really holds
        std::vector<u64> held(D);
        for (size_t t = 0; t < batch; t++) {
            const u32 len = bucket_tile_len(total, tile, t);
            if (!len) continue;
            std::vector<u64> before(D, 0);
            for (u32 w = 0; w < BUCKET_WAVES; w++) {
                u32 b, e;
                bucket_wave_run(tile, len, w, &b, &e);
                std::fill(held.begin(), held.end(), 0);
                for (u32 r = b; r < e; r++) held[bucket_digit(a.in[0][t * tile + r], shift, width)]++;
                for (size_t d = 0; d < D; d++) {
                    const u64 sc = a.in[2][d * batch + t];
                    if (held[d]) need(sc <= room && before[d] <= room - sc && held[d] <= room - sc - before[d], "bucket_scatter: a target place at or beyond the room of out[0]");
                    before[d] += a.in[3][(t * BUCKET_WAVES + w) * D + d];
                }
            }
        }
    } break;
    case STEP_BUCKET_OFFSETS:
    case STEP_BUCKET_ORDER: {
        // in[0] the ascending keys (null or empty with a total of 0), in[1] total; OFFSETS: terms = T -> out[0] [T + 2]; ORDER -> out[0] [room]
        const size_t given = a.in[0] ? a.in_words[0] : 0;
        in_is(1, 1, "bucket_offsets / bucket_order: in[1] total, one word");
        total = a.in[1][0];
        need(total <= given, "bucket_offsets / bucket_order: a total above the keys given");
        if (a.step == STEP_BUCKET_OFFSETS) {
            T = terms;
            need(T >= 1, "bucket_offsets: T (terms) of 0");
            out_is(0, T + 2, "bucket_offsets: out[0] [T + 2]");
            for (u64 k = 1; k < total; k++) need(a.in[0][k - 1] <= a.in[0][k], "bucket_offsets: the keys below total do not ascend");
        } else {
            need(a.out[0] && a.out_words[0] >= 1 && total <= a.out_words[0], "bucket_order: out[0] [room], total <= room: wrong size");
            room = a.out_words[0];
            fits32(a.out[0], room, "bucket_order: out[0]");
        }
    } break;
    default: {                                                         // STEP_ENTRIES_GATHER
        // batch = room; in[0] items [count][2], in[1] order [room], in[2] total -> out[0] [room][2]
        room = batch;
        need(room >= 1, "entries_gather: room (batch) of 0");
        need(a.in[0] && a.in_words[0] >= 2 && a.in_words[0] % 2 == 0, "entries_gather: in[0] items [count][2], count >= 1: wrong size");
        count = a.in_words[0] / 2;
        in_is(1, room, "entries_gather: in[1] order [room]");
        in_is(2, 1, "entries_gather: in[2] total, one word");
        out_is(0, 2 * room, "entries_gather: out[0] [room][2]");
        total = a.in[2][0];
        need(total <= room, "entries_gather: a total above the room");
        for (u64 k = 0; k < total; k++) need(a.in[1][k] < count, "entries_gather: an order word below total names no item");
    } break;
    }

    // host copies of the narrowed arrays and the widening of what comes back: both outlive the queued copies (the call ends with a sync)
    std::list<std::vector<u32>> keep32;
    std::vector<std::function<void()>> after;

    WITH_ARENA({
        keep32.clear(); after.clear();                                 // a retry with a larger arena starts over
        auto up = [&](const u64 *src, size_t words) {
            u64 *d = ws(words + 2);
            if (words) HIP_CHECK(hipMemcpyAsync(d, src, words * sizeof(u64), hipMemcpyHostToDevice, st_));
            return d;
        };
        auto up32 = [&](const u64 *src, size_t words) {
            keep32.emplace_back(words);
            std::vector<u32> &h = keep32.back();
            for (size_t i = 0; i < words; i++) h[i] = (u32)src[i];
            u32 *d = ws_as<u32>(words, 1);
            if (words) HIP_CHECK(hipMemcpyAsync(d, h.data(), words * sizeof(u32), hipMemcpyHostToDevice, st_));
            return d;
        };
        auto down = [&](u64 *dst, const u64 *src, size_t words) { if (words) HIP_CHECK(hipMemcpyAsync(dst, src, words * sizeof(u64), hipMemcpyDeviceToHost, st_)); };
        auto down32 = [&](u64 *dst, const u32 *src, size_t words) {
            keep32.emplace_back(words);
            std::vector<u32> *h = &keep32.back();
            if (words) HIP_CHECK(hipMemcpyAsync(h->data(), src, words * sizeof(u32), hipMemcpyDeviceToHost, st_));
            after.push_back([=] { for (size_t i = 0; i < words; i++) dst[i] = (*h)[i]; });
        };

        switch (a.step) {
        case STEP_BUCKET_COUNT: {
            const u32 *dlocs = up32(a.in[0], a.in_words[0]);
            u32 *dcnt = up32(a.out[0], key_tiles);
            launch_bucket_count(dlocs, count, H, tile, dcnt, st_);
            down32(a.out[0], dcnt, key_tiles);
        } break;
        case STEP_BUCKET_KEYS: {
            const u32 *dlocs = up32(a.in[0], a.in_words[0]);
            const u64 *dbase = up(a.in[1], key_tiles);
            u64 *dkeys = up(a.out[0], room);
            launch_bucket_keys(dlocs, count, H, tile, dbase, dkeys, st_);
            down(a.out[0], dkeys, room);
        } break;
        case STEP_BUCKET_SCAN: {
            const u32 *din = up32(a.in[0], n);
            u64 *dout = up(a.out[0], n + 1);
            u64 *dsum = a.flags & STEP_STORE ? up(a.out[1], 1) : nullptr;
            launch_bucket_scan(din, n, dout, dsum, st_);
            down(a.out[0], dout, n + 1);
            if (dsum) down(a.out[1], dsum, 1);
        } break;
        case STEP_BUCKET_HIST: {
            const u64 *dkeys = up(a.in[0], a.in_words[0]), *dtotal = up(a.in[1], 1);
            u32 *dhist = up32(a.out[0], a.out_words[0]), *dwc = up32(a.out[1], a.out_words[1]);
            launch_bucket_hist(dkeys, dtotal, batch, tile, shift, width, dhist, dwc, st_);
            down32(a.out[0], dhist, a.out_words[0]);
            down32(a.out[1], dwc, a.out_words[1]);
        } break;
        case STEP_BUCKET_SCATTER: {
            const u64 *dkeys = up(a.in[0], a.in_words[0]), *dtotal = up(a.in[1], 1), *dscanned = up(a.in[2], a.in_words[2]);
            const u32 *dwc = up32(a.in[3], a.in_words[3]);
            u64 *dout = up(a.out[0], room);
            launch_bucket_scatter(dkeys, dtotal, batch, tile, shift, width, dscanned, dwc, dout, st_);
            down(a.out[0], dout, room);
        } break;
        case STEP_BUCKET_OFFSETS: {
            const u64 *dkeys = up(a.in[0], a.in[0] ? a.in_words[0] : 0), *dtotal = up(a.in[1], 1);      // (the words behind total go up too)
            u64 *doff = up(a.out[0], T + 2);
            launch_bucket_offsets(dkeys, dtotal, (u32)T, doff, st_);
            down(a.out[0], doff, T + 2);
        } break;
        case STEP_BUCKET_ORDER: {
            const u64 *dkeys = up(a.in[0], a.in[0] ? a.in_words[0] : 0), *dtotal = up(a.in[1], 1);
            u32 *dorder = up32(a.out[0], room);
            launch_bucket_order(dkeys, dtotal, room, dorder, st_);
            down32(a.out[0], dorder, room);
        } break;
        default: {                                                     // STEP_ENTRIES_GATHER
            const u64 *ditems = up(a.in[0], a.in_words[0]), *dtotal = up(a.in[2], 1);
            const u32 *dorder = up32(a.in[1], room);
            u64 *dent = up(a.out[0], 2 * room);
            launch_entries_gather(reinterpret_cast<const unsigned char *>(ditems), dorder, dtotal, room, reinterpret_cast<unsigned char *>(dent), st_);
            down(a.out[0], dent, 2 * room);
        } break;
        }
        sync();
        for (auto &f : after) f();
    });
}

} // namespace apsu_he
