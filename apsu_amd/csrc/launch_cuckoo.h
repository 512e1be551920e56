// Launch entry points of kernels_cuckoo.hip: item locations, the querier's cuckoo table and its slot values.  Rules: cuckoo.h.
#pragma once
#include <hip/hip_runtime.h>
#include "cuckoo.h"

namespace apsu_he {

// locs[count][H] = loc_f(item i) for f < H, tabs: [H][16][256] words on the device (cuckoo_tables).
// contract: items 16-byte aligned, count * 16 bytes; 1 <= H <= CUCKOO_MAX_FUNCS; T >= 1.  Exactly count * H words are written.
// Persistent workgroups of CUCKOO_LOC_T lanes; the tables go through LDS cuckoo_group(H) functions at a time, interleaved (cuckoo_hash_group)
// and staged once per workgroup and group; `wgs` caps the grid (0: two workgroups per compute unit of the current device).
void launch_cuckoo_locations(const unsigned char *items, size_t count, const u32 *tabs, u32 H, u32 T, u32 *locs, u32 wgs, hipStream_t st);

// The table rule of cuckoo.h in one workgroup.  items [count][16] (any alignment), locs [count][H] words below T, 1 <= H, T >= 1,
// 1 <= max_rounds <= CUCKOO_MAX_ROUNDS, count < 2^32 - 1.  lds_table: the T slots live in LDS (T <= CUCKOO_LDS_SLOTS, else
// std::logic_error and nothing is launched), else in `table` (T words of device memory; not read or written by the LDS form).
// state, prop_round: count words of scratch each.  Outputs: table_idx[T] (item or CUCKOO_NONE), item_loc[count] (location, CUCKOO_NONE
// for a duplicate; of an unplaced item: the location it last lost), status[3] = rounds run, the lowest unplaced item (~0: none),
// the items placed.  Both forms give the same words.
void launch_cuckoo_insert(bool lds_table, const unsigned char *items, const u32 *locs, u32 count, u32 H, u32 T, u64 max_rounds, u64 *table,
                          u32 *state, u32 *prop_round, u32 *table_idx, u32 *item_loc, u64 *status, hipStream_t st);

// values[nb][n] of the querier's table after the caller's OPRF (query_value_slot, cuckoo_item_felt): table_items [nb * items_per_bundle][16],
// 8-byte aligned.  contract: F >= 1, items_per_bundle * F <= n, nb <= 65535; exactly nb * n words are written.
void launch_query_values(const unsigned char *table_items, u32 nb, u32 items_per_bundle, u32 F, u32 bpf, u32 item_bits, size_t n, u64 *values,
                         hipStream_t st);

} // namespace apsu_he
