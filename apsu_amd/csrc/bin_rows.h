// The bins' polynomials of a resident BinBundle as ragged rows (Engine::export_saved, k_bins_rows): the index rules of one lane and
// the pure host functions, no HIP in here.  With poly[d][slot] the decoded array of a BinBundle (Engine::decode_bundle; rows above a
// slot's count are 0, the row at the count is 1) and count[s] from k_bin_counts, the matching polynomial of bin s is the column s
// read from row 0 to row count[s]: ascending and monic, [1] for an empty bin.  A saved BinBundle (bin_bundle.fbs:
// cache.felt_matching_polyns) wants these columns as rows of their own length, one behind the other:
//   out[off[s] + d] = poly[d][s],  d <= count[s],  off = the exclusive scan of count[s] + 1 over the bins.
// The kernel runs the functions below, the CPU emulation (emu/db.cpp: emu_bins_rows) the same loop structure with an explicit loop
// over the workgroup's waves and their 64 lanes (tests/test_saved_db_writer_cpu.py).
//
// k_bins_rows is a transposition through LDS and nothing else: no arithmetic, no atomics.  A workgroup of ROWS_WAVES waves owns a
// tile of 64 consecutive slots x 64 consecutive degrees.  Loading, lane = slot: wave w reads the row segments poly[d0 + w + 4 i][s0 ..
// s0 + 63], 512 contiguous bytes each -- no lane walks down a column, whose stride is 8 n bytes (the rule k_bins_lookup and
// k_bins_merge keep).  Storing, lane = degree: wave w takes the slots s0 + w + 4 i and writes out[off[s] + d0 + lane] for the lanes
// with d0 + lane <= count[s], again contiguous.  The tile is padded by one word per degree row: the transposed read of lane l is at
// word l * 65 + s, that is at dword bank (2 l + 2 s) mod 64 for ds_read_b64's 64-dword bank row, so the 32 lanes of a half-wave hit
// 32 different bank pairs; unpadded they would all hit one.  A tile whose largest count is below d0 is left at once (the tops are
// merge_tile_tops' of the counts), so a tile of short bins does not read the BinBundle's tallest rows.
#pragma once
#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

#include "bin_lookup.h"

namespace apsu_he {

constexpr int ROWS_TILE = 64;                             // slots and degrees per tile = lanes per wave
constexpr int ROWS_WAVES = 4;                             // waves per workgroup (resource report: profiles/r16_saved_export.txt)
constexpr int ROWS_PAD = 1;                               // words behind every degree row of the LDS tile
constexpr int ROWS_LDS_WORDS = ROWS_TILE * (ROWS_TILE + ROWS_PAD);
static_assert(ROWS_TILE % ROWS_WAVES == 0, "every wave takes the same number of rows");

// word of the LDS tile that holds (degree d0 + dl, slot s0 + sl)
HD int rows_lds_at(int dl, int sl) { return dl * (ROWS_TILE + ROWS_PAD) + sl; }
// the load of (degree d, slot s) happens: inside the array and not above the tile's largest count
HD bool rows_load_live(u32 d, size_t s, u32 rows, size_t n, int top) { return s < n && d < rows && (int)d <= top; }
// the store of (degree d, slot s) happens: s is one of the `bins` bins and d is a coefficient of its polynomial
HD bool rows_store_live(u32 d, size_t s, u32 count, u32 bins) { return s < bins && count != LOOKUP_NONE && d <= count; }

// off[bins + 1]: where each bin's row starts, off[bins] = the words of all rows.  Every one of the `bins` first slots must be a bin
// (a slot that holds the zero polynomial has no matching polynomial to write) and no count may exceed the array: std::invalid_argument
// names the slot.
inline std::vector<u64> rows_offsets(const u32 *counts, u32 bins, u32 rows)
{
    std::vector<u64> off((size_t)bins + 1, 0);
    for (u32 s = 0; s < bins; s++) {
        if (counts[s] == LOOKUP_NONE)
            throw std::invalid_argument("bin " + std::to_string(s) + " is an unused slot (it holds the zero polynomial): it has no matching polynomial");
        if (counts[s] >= rows)
            throw std::invalid_argument("bin " + std::to_string(s) + ": count " + std::to_string(counts[s]) + " exceeds the BinBundle's degree");
        off[s + 1] = off[s] + counts[s] + 1;
    }
    return off;
}

// per tile of 64 slots the largest count among the first `bins` slots, -1 for a tile without one
inline std::vector<int> rows_tile_tops(const u32 *counts, size_t n, u32 bins)
{
    std::vector<int> tops((n + ROWS_TILE - 1) / ROWS_TILE, -1);
    for (size_t s = 0; s < n && s < bins; s++)
        if (counts[s] != LOOKUP_NONE && (int)counts[s] > tops[s / ROWS_TILE]) tops[s / ROWS_TILE] = (int)counts[s];
    return tops;
}

}  // namespace apsu_he
