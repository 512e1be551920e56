// See engine.h.  Cuckoo hashing for both parties (cuckoo.h): every item's locations and the database side's grouping by location, the
// querier's table and its slot values.  Shares the arena and the stream with the other calls (engine_impl.h).
#include "engine_impl.h"
#include "launch_cuckoo.h"
#include "launch_bucket.h"

namespace apsu_he {

// the location functions' tables, made by the first call that hashes (an allocation at creation would move every buffer behind it)
void Engine::cuckoo_tables_ready()
{
    if (d_cuckoo_tabs_.bytes()) return;
    const u32 H = psu_.table_params.hash_func_count;
    std::vector<u32> tabs((size_t)H * CUCKOO_TAB_WORDS);
    for (u32 f = 0; f < H; f++) cuckoo_tables(f, tabs.data() + (size_t)f * CUCKOO_TAB_WORDS);
    DevBuf d(tabs.size() * sizeof(u32));
    HIP_CHECK(hipMemcpyAsync(d.p(), tabs.data(), tabs.size() * sizeof(u32), hipMemcpyHostToDevice, st_));
    sync();
    d_cuckoo_tabs_ = std::move(d);
}

// caller items as 16-byte aligned device memory: the caller's own pointer where it is one, else a copy in the arena
const unsigned char *Engine::cuckoo_items(const unsigned char *items, size_t count, bool on_device)
{
    if (on_device && !((uintptr_t)items & 15)) return items;
    unsigned char *d = ws_as<unsigned char>(count * 16 + 16);
    if (count) HIP_CHECK(hipMemcpyAsync(d, items, count * 16, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st_));
    return d;
}

void Engine::item_locations(const unsigned char *items, size_t count, bool items_on_device, uint32_t *locs, bool locs_on_device)
{
    Enter g(this);
    lookup_check(nullptr, NEED_PSU);
    if (!count) return;
    cuckoo_tables_ready();
    TIER1_SLOTS();
    const u32 H = psu_.table_params.hash_func_count, T = psu_.table_params.table_size;
    WITH_ARENA({
        const unsigned char *src = cuckoo_items(items, count, items_on_device);
        u32 *dst = locs_on_device ? locs : ws_as<u32>(count * H);
        { PROF(P_OTHER, 0); launch_cuckoo_locations(src, count, reinterpret_cast<const u32 *>(d_cuckoo_tabs_.p()), H, T, dst, 0, st_); }
        if (!locs_on_device) HIP_CHECK(hipMemcpyAsync(locs, dst, count * H * sizeof(u32), hipMemcpyDeviceToHost, st_));
        sync();
    });
}

void Engine::debug_item_locations(const unsigned char *items, size_t count, uint32_t H, uint32_t T, uint32_t *locs)
{
    Enter g(this);
    if (!H || H > CUCKOO_MAX_FUNCS || !T) throw std::invalid_argument("debug_item_locations: 1 <= H <= 8 and T >= 1");
    if (!count) return;
    std::vector<u32> tabs((size_t)H * CUCKOO_TAB_WORDS);
    for (u32 f = 0; f < H; f++) cuckoo_tables(f, tabs.data() + (size_t)f * CUCKOO_TAB_WORDS);
    TIER1_SLOTS();
    WITH_ARENA({
        const unsigned char *src = cuckoo_items(items, count, false);
        u32 *dtabs = ws_as<u32>(tabs.size()), *dst = ws_as<u32>(count * H);
        HIP_CHECK(hipMemcpyAsync(dtabs, tabs.data(), tabs.size() * sizeof(u32), hipMemcpyHostToDevice, st_));
        { PROF(P_OTHER, 0); launch_cuckoo_locations(src, count, dtabs, H, T, dst, 0, st_); }
        HIP_CHECK(hipMemcpyAsync(locs, dst, count * H * sizeof(u32), hipMemcpyDeviceToHost, st_));
        sync();
    });
}

void Engine::items_bucket(const unsigned char *items, size_t count, bool items_on_device, u64 *offsets, uint32_t *order, u64 *total)
{
    if (count >= CUCKOO_NONE) throw std::invalid_argument("items_bucket: more items than a 32-bit index names");
    u32 H, T;
    {
        Enter g(this);
        lookup_check(nullptr, NEED_PSU);
        H = psu_.table_params.hash_func_count; T = psu_.table_params.table_size;
    }
    std::vector<u32> locs(count * H);
    item_locations(items, count, items_on_device, locs.data(), false);
    if (!cuckoo_bucket(locs.data(), count, H, T, offsets, order, total)) throw std::runtime_error("items_bucket: a location outside the table");
}

// ---- the grouping on the device (bucket_plan.h, kernels_bucket.hip).  Inside WITH_ARENA: dlocs [count][H] -> offsets [T + 1] and the
// total in the arena, order [count * H] where the caller says; everything is queued, nothing waited for
Engine::BucketOut Engine::bucket_run(const u32 *dlocs, size_t count, u32 H, u32 T, u32 tile, u32 *dorder)
{
    const BucketSizes s = bucket_sizes(count, H, T, tile);
    BucketWork w{};
    w.keys[0] = ws(s.keys);
    w.keys[1] = ws(s.keys);
    w.tile_cnt = ws_as<u32>(s.tile_cnt);
    w.tile_base = ws(s.tile_base);
    w.hist = ws_as<u32>(s.hist);
    w.wave_cnt = ws_as<u32>(s.wave_cnt);
    w.scanned = ws(s.scanned);
    w.total = ws(1);
    BucketOut out{};
    out.offsets = ws((size_t)T + 1);
    out.total = w.total;
    { PROF(P_OTHER, 0); launch_bucket_sort(dlocs, count, H, T, tile, w, out.offsets, dorder, st_); }
    return out;
}

void Engine::items_bucket_device(const unsigned char *items, size_t count, bool items_on_device, u64 *offsets, uint32_t *order, bool order_on_device,
                                 unsigned char *entries, bool entries_on_device, u64 *total)
{
    if (count >= CUCKOO_NONE) throw std::invalid_argument("items_bucket_device: more items than a 32-bit index names");
    Enter g(this);
    lookup_check(nullptr, NEED_PSU);
    const u32 H = psu_.table_params.hash_func_count, T = psu_.table_params.table_size;
    OpClock &clk = clock_[OP_BUCKET];
    for (double &m : clk.ms) m = 0;
    for (size_t l = 0; l <= T; l++) offsets[l] = 0;
    *total = 0;
    if (!count) return;
    cuckoo_tables_ready();
    TIER1_SLOTS();
    clk.evs.reserve(4);                                                // around the locations, the grouping and the gather
    const u64 room = (u64)count * H;
    WITH_ARENA({
        const unsigned char *src = cuckoo_items(items, count, items_on_device);
        u32 *dlocs = ws_as<u32>(room);
        u32 *dorder = order && order_on_device ? order : ws_as<u32>(room);
        unsigned char *dent = !entries ? nullptr : entries_on_device && !((uintptr_t)entries & 15) ? entries : ws_as<unsigned char>(room * 16 + 16);
        clk.evs.record(0, st_);
        { PROF(P_OTHER, 0); launch_cuckoo_locations(src, count, reinterpret_cast<const u32 *>(d_cuckoo_tabs_.p()), H, T, dlocs, 0, st_); }
        clk.evs.record(1, st_);
        const BucketOut out = bucket_run(dlocs, count, H, T, BUCKET_TILE_DEFAULT, dorder);
        clk.evs.record(2, st_);
        if (dent) { PROF(P_OTHER, 0); launch_entries_gather(src, dorder, out.total, room, dent, st_); }
        clk.evs.record(3, st_);
        HIP_CHECK(hipMemcpyAsync(offsets, out.offsets, ((size_t)T + 1) * sizeof(u64), hipMemcpyDeviceToHost, st_));
        sync();
        const u64 n = offsets[T];
        if (order && !order_on_device && n) HIP_CHECK(hipMemcpyAsync(order, dorder, n * sizeof(u32), hipMemcpyDeviceToHost, st_));
        if (entries && dent != entries && n) HIP_CHECK(hipMemcpyAsync(entries, dent, n * 16, entries_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st_));
        sync();
    });
    *total = offsets[T];
    for (int k = 0; k < 3; k++) clk.ms[k] = clk.evs.ms(k, k + 1);
}

void Engine::debug_bucket_locs(const uint32_t *locs, size_t count, uint32_t H, uint32_t T, uint32_t tile, u64 *offsets, uint32_t *order, u64 *total)
{
    Enter g(this);
    if (!H || H > CUCKOO_MAX_FUNCS || !T) throw std::invalid_argument("debug_bucket_locs: 1 <= H <= 8 and T >= 1");
    if (count >= CUCKOO_NONE) throw std::invalid_argument("debug_bucket_locs: more items than a 32-bit index names");
    if (!tile) tile = BUCKET_TILE_DEFAULT;
    if (!bucket_tile_ok(tile))
        throw std::invalid_argument("debug_bucket_locs: tile_entries must be a multiple of " + std::to_string(BUCKET_TILE_STEP) + " in [" +
                                    std::to_string(BUCKET_TILE_MIN) + ", " + std::to_string(BUCKET_TILE_MAX) + "]");
    for (size_t k = 0; k < count * H; k++)
        if (locs[k] >= T) throw std::invalid_argument("debug_bucket_locs: location " + std::to_string(k) + " is outside the table");
    OpClock &clk = clock_[OP_BUCKET];
    for (double &m : clk.ms) m = 0;
    for (size_t l = 0; l <= T; l++) offsets[l] = 0;
    *total = 0;
    if (!count) return;
    TIER1_SLOTS();
    clk.evs.reserve(4);
    WITH_ARENA({
        u32 *dlocs = ws_as<u32>(count * H);
        u32 *dorder = ws_as<u32>(count * H);
        HIP_CHECK(hipMemcpyAsync(dlocs, locs, count * H * sizeof(u32), hipMemcpyHostToDevice, st_));
        clk.evs.record(1, st_);
        const BucketOut out = bucket_run(dlocs, count, H, T, tile, dorder);
        clk.evs.record(2, st_);
        HIP_CHECK(hipMemcpyAsync(offsets, out.offsets, ((size_t)T + 1) * sizeof(u64), hipMemcpyDeviceToHost, st_));
        sync();
        if (offsets[T]) HIP_CHECK(hipMemcpyAsync(order, dorder, offsets[T] * sizeof(u32), hipMemcpyDeviceToHost, st_));
        sync();
    });
    *total = offsets[T];
    clk.ms[1] = clk.evs.ms(1, 2);
}

void Engine::cuckoo_insert_run(const unsigned char *ditems, const u32 *dlocs, u32 count, u32 H, u32 T, u64 max_rounds, int form, uint32_t *table_idx,
                               uint32_t *item_loc, u64 *rounds)
{
    const bool lds = form == CUCKOO_FORM_LDS || (form == CUCKOO_FORM_AUTO && T <= CUCKOO_LDS_SLOTS);
    u64 *table = lds ? nullptr : ws(T);
    u32 *state = ws_as<u32>((size_t)count + 1), *prop = ws_as<u32>((size_t)count + 1);
    u32 *d_idx = ws_as<u32>(T), *d_loc = ws_as<u32>((size_t)count + 1);
    u64 *d_status = ws(3);
    { PROF(P_OTHER, 0); launch_cuckoo_insert(lds, ditems, dlocs, count, H, T, max_rounds, table, state, prop, d_idx, d_loc, d_status, st_); }
    u64 status[3];
    HIP_CHECK(hipMemcpyAsync(status, d_status, sizeof(status), hipMemcpyDeviceToHost, st_));
    sync();
    if (status[1] != ~(u64)0) {
        char rate[32];
        snprintf(rate, sizeof(rate), "%.3f", (double)status[2] / (double)T);
        throw std::runtime_error("cuckoo table: item " + std::to_string(status[1]) + " is the lowest of those without a slot after " +
                                 std::to_string(status[0]) + " rounds (fill rate " + rate + ")");
    }
    HIP_CHECK(hipMemcpyAsync(table_idx, d_idx, (size_t)T * sizeof(u32), hipMemcpyDeviceToHost, st_));
    if (count) HIP_CHECK(hipMemcpyAsync(item_loc, d_loc, (size_t)count * sizeof(u32), hipMemcpyDeviceToHost, st_));
    sync();
    if (rounds) *rounds = status[0];
}

static void check_rounds(u64 max_rounds)
{
    if (!max_rounds || max_rounds > CUCKOO_MAX_ROUNDS) throw std::invalid_argument("max_rounds must be in [1, 2^32]");
}

void Engine::cuckoo_table(const unsigned char *items, size_t count, bool items_on_device, u64 max_rounds, uint32_t *table_idx, uint32_t *item_loc,
                          u64 *rounds)
{
    Enter g(this);
    lookup_check(nullptr, NEED_PSU);
    check_rounds(max_rounds);
    if (count >= CUCKOO_NONE) throw std::invalid_argument("cuckoo_table: more items than a 32-bit index names");
    cuckoo_tables_ready();
    TIER1_SLOTS();
    const u32 H = psu_.table_params.hash_func_count, T = psu_.table_params.table_size;
    WITH_ARENA({
        const unsigned char *src = cuckoo_items(items, count, items_on_device);
        u32 *dlocs = ws_as<u32>(count * H + 1);
        { PROF(P_OTHER, 0); launch_cuckoo_locations(src, count, reinterpret_cast<const u32 *>(d_cuckoo_tabs_.p()), H, T, dlocs, 0, st_); }
        cuckoo_insert_run(src, dlocs, (u32)count, H, T, max_rounds, CUCKOO_FORM_AUTO, table_idx, item_loc, rounds);
    });
}

void Engine::debug_cuckoo_insert(const unsigned char *items, const uint32_t *locs, size_t count, uint32_t H, uint32_t T, u64 max_rounds, int form,
                                 uint32_t *table_idx, uint32_t *item_loc, u64 *rounds)
{
    Enter g(this);
    check_rounds(max_rounds);
    if (!H || H > CUCKOO_MAX_FUNCS || !T) throw std::invalid_argument("debug_cuckoo_insert: 1 <= H <= 8 and T >= 1");
    if (form < CUCKOO_FORM_AUTO || form > CUCKOO_FORM_GLOBAL) throw std::invalid_argument("debug_cuckoo_insert: no such table form");
    if (count >= CUCKOO_NONE) throw std::invalid_argument("debug_cuckoo_insert: more items than a 32-bit index names");
    for (size_t k = 0; k < count * H; k++)
        if (locs[k] >= T) throw std::invalid_argument("debug_cuckoo_insert: location " + std::to_string(k) + " is outside the table");
    if (form == CUCKOO_FORM_LDS && T > CUCKOO_LDS_SLOTS)
        throw std::logic_error("the cuckoo table does not fit LDS: " + std::to_string(T) + " slots, " + std::to_string(CUCKOO_LDS_SLOTS) + " fit");
    TIER1_SLOTS();
    WITH_ARENA({
        const unsigned char *src = cuckoo_items(items, count, false);
        u32 *dlocs = ws_as<u32>(count * H + 1);
        if (count) HIP_CHECK(hipMemcpyAsync(dlocs, locs, count * H * sizeof(u32), hipMemcpyHostToDevice, st_));
        cuckoo_insert_run(src, dlocs, (u32)count, H, T, max_rounds, form, table_idx, item_loc, rounds);
    });
}

void Engine::query_values(const unsigned char *table_items, bool on_device, u64 *values, bool values_on_device)
{
    Enter g(this);
    lookup_check("query_values", NEED_PSU);
    TIER1_SLOTS();
    const u32 T = psu_.table_params.table_size, nb = psu_.bundle_idx_count, ipb = psu_.items_per_bundle;
    const u32 F = psu_.item_params.felts_per_item, bpf = psu_.item_bit_count_per_felt, bits = psu_.item_bit_count;
    const size_t n = hp_.n;
    WITH_ARENA({
        const unsigned char *src = cuckoo_items(table_items, T, on_device);
        u64 *dst = values_on_device ? values : ws((size_t)nb * n);
        { PROF(P_OTHER, 0); launch_query_values(src, nb, ipb, F, bpf, bits, n, dst, st_); }
        if (!values_on_device) HIP_CHECK(hipMemcpyAsync(values, dst, (size_t)nb * n * sizeof(u64), hipMemcpyDeviceToHost, st_));
        sync();
    });
}

} // namespace apsu_he
