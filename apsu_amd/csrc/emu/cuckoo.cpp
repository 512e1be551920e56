// CPU emulation, cuckoo hashing (cuckoo.h: the functions kernels_cuckoo.hip runs; model: tests/cuckoo_model.py)
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "emu_common.h"
#include "cuckoo.h"

using namespace apsu_he;

extern "C" {

// tab[16][256] of location function f
void emu_cuckoo_tables(uint32_t f, uint32_t *tab) { cuckoo_tables(f, tab); }

// locs[count][H] of items [count][16] in a table of T slots
int emu_cuckoo_locations(const uint8_t *items, uint64_t count, uint32_t H, uint32_t T, uint32_t *locs)
{
    return guarded([&]() -> int {
        if (!H || H > CUCKOO_MAX_FUNCS || !T) throw std::invalid_argument("1 <= H <= 8 and T >= 1");
        std::vector<u32> tab(CUCKOO_TAB_WORDS);
        for (u32 f = 0; f < H; f++) {
            cuckoo_tables(f, tab.data());
            for (size_t i = 0; i < count; i++) locs[i * H + f] = cuckoo_loc(tab.data(), items + i * 16, T);
        }
        // once more as k_cuckoo_locations computes them: the staged, interleaved image of each group and cuckoo_hash_group
        std::vector<u32> tabs((size_t)H * CUCKOO_TAB_WORDS);
        for (u32 f = 0; f < H; f++) cuckoo_tables(f, tabs.data() + (size_t)f * CUCKOO_TAB_WORDS);
        const u32 G = cuckoo_group(H);
        std::vector<u32> img((size_t)G * CUCKOO_TAB_WORDS);
        for (u32 g0 = 0; g0 < H; g0 += G) {
            const u32 ng = std::min(G, H - g0);
            for (u32 idx = 0; idx < G * CUCKOO_TAB_WORDS; idx++)
                img[cuckoo_group_image(idx, G)] = idx < ng * CUCKOO_TAB_WORDS ? tabs[(size_t)g0 * CUCKOO_TAB_WORDS + idx] : 0;
            for (size_t i = 0; i < count; i++) {
                u32 w[4], x[4] = { 0, 0, 0, 0 };
                std::memcpy(w, items + i * 16, 16);
                if (G == 1) cuckoo_hash_group<1>(img.data(), w[0], w[1], w[2], w[3], x);
                else if (G == 2) cuckoo_hash_group<2>(img.data(), w[0], w[1], w[2], w[3], x);
                else cuckoo_hash_group<4>(img.data(), w[0], w[1], w[2], w[3], x);
                for (u32 g = 0; g < ng; g++)
                    if (x[g] % T != locs[i * H + g0 + g]) throw std::logic_error("the grouped hash differs from cuckoo_loc");
            }
        }
        return 0;
    });
}

// The table rule with k_cuckoo_insert's phases as explicit loops over the items: propose, the barrier, settle.  table_idx[T],
// item_loc[count], *rounds = rounds run.  -> 0, or 1 with *unplaced = the lowest item without a slot after max_rounds and *placed = the
// slots taken (then table_idx and item_loc mean nothing), or -1.
int emu_cuckoo_insert(const uint8_t *items, const uint32_t *locs, uint64_t count, uint32_t H, uint32_t T, uint64_t max_rounds, uint32_t *table_idx,
                      uint32_t *item_loc, uint64_t *rounds, uint64_t *unplaced, uint64_t *placed)
{
    return guarded([&]() -> int {
        if (!H || !T || !max_rounds || max_rounds > CUCKOO_MAX_ROUNDS || count >= CUCKOO_NONE) throw std::invalid_argument("outside the rule's ranges");
        for (size_t k = 0; k < count * H; k++) if (locs[k] >= T) throw std::invalid_argument("location outside the table");
        std::vector<u64> table(T, CUCKOO_EMPTY);
        std::vector<u32> state(count, CUCKOO_ACTIVE), h(count, 0), prop(count, 0);
        u64 r = 0;
        bool more = count != 0;
        while (more && r < max_rounds) {
            for (size_t i = 0; i < count; i++) {
                if (state[i] != CUCKOO_ACTIVE) continue;
                u64 &slot = table[locs[i * H + h[i]]];
                slot = std::min(slot, cuckoo_key(max_rounds, r, (u32)i));
                prop[i] = (u32)r;
            }
            more = false;
            for (size_t i = 0; i < count; i++) {
                if (state[i] == CUCKOO_DUPLICATE) continue;
                const u64 own = cuckoo_key(max_rounds, prop[i], (u32)i), v = table[locs[i * H + h[i]]];
                const bool eq = v != own && cuckoo_items_equal(items + (size_t)cuckoo_key_item(v) * 16, items + i * 16);
                state[i] = cuckoo_settle(own, v, eq);
                if (state[i] == CUCKOO_ACTIVE) { h[i] = (h[i] + 1) % H; more = true; }
            }
            r++;
        }
        *rounds = r; *unplaced = ~(u64)0; *placed = 0;
        for (size_t i = count; i-- > 0;) { if (state[i] == CUCKOO_ACTIVE) *unplaced = i; *placed += state[i] == CUCKOO_PLACED; }
        if (*unplaced != ~(u64)0) return 1;
        for (u32 s = 0; s < T; s++) table_idx[s] = table[s] == CUCKOO_EMPTY ? CUCKOO_NONE : cuckoo_key_item(table[s]);
        for (size_t i = 0; i < count; i++) item_loc[i] = state[i] == CUCKOO_DUPLICATE ? CUCKOO_NONE : locs[i * H + h[i]];
        return 0;
    });
}

// the database side's grouping (cuckoo_bucket): offsets[T + 1], order[count * H]
int emu_bucket_items(const uint32_t *locs, uint64_t count, uint32_t H, uint32_t T, uint64_t *offsets, uint32_t *order, uint64_t *total)
{
    return cuckoo_bucket(locs, count, H, T, offsets, order, total) ? 0 : -1;
}

// k_query_values lane by lane: values[nb][n] of table_items [nb * items_per_bundle][16]
void emu_query_values(const uint8_t *table_items, uint32_t nb, uint32_t items_per_bundle, uint32_t F, uint32_t bpf, uint32_t item_bits, uint64_t n,
                      uint64_t *values)
{
    for (u32 b = 0; b < nb; b++)
        for (size_t p = 0; p < n; p++) {
            u32 j = 0;
            const u32 slot = query_value_slot(b, (u32)p, items_per_bundle, F, &j);
            u64 w[2] = { 0, 0 };
            if (slot != CUCKOO_NONE) std::memcpy(w, table_items + (size_t)slot * 16, 16);
            values[(size_t)b * n + p] = slot == CUCKOO_NONE ? 0 : cuckoo_item_felt(w[0], w[1], j, bpf, item_bits);
        }
}

int emu_cuckoo_lds_slots() { return (int)CUCKOO_LDS_SLOTS; }

} // extern "C"
