// Asking a resident BinBundle's polynomials questions (Engine::lookup_bundles, k_bin_counts, k_bins_lookup): the arithmetic of one lane
// and the pure host functions, no HIP in here.  The kernels run the lane functions on the decoded poly[d][slot] (Engine::decode_bundle),
// the CPU emulation (emu/db.cpp: emu_bin_counts, emu_bins_lookup) runs the kernels' loop structure with an explicit loop over the 64
// lanes (tests/test_bundle_lookup_cpu.py).
//
// An entry is felts_per_item field elements f_0 .. f_{F-1} and a start bin s; part j belongs to bin (slot) s + j.  Part j is found iff
// P_{s+j}(f_j) = 0 mod t and the slot is a bin, i.e. does not hold the zero polynomial (where Horner gives 0 for every point).
//
// k_bins_lookup has lane = slot: a wave owns a tile of 64 consecutive slots and walks the rows d = degree .. 0, one contiguous
// 512-byte row segment per d, with up to R points per lane in registers.  So the points must reach it grouped by slot.  lookup_plan
// lays them out as rows of 64 words: row r of a tile holds, in lane l, the r-th point of slot 64 tile + l (or nothing: idx = NONE),
// and the tile has as many rows as its fullest slot has points.  The rows of all tiles are concatenated; a work item is (tile, first
// row, number of rows <= R).  Storage is 64 words per row and there are never more rows than parts, whatever the skew: a batch whose
// entries all start at one bin makes many work items for one tile and none for the others.
#pragma once
#include <cstddef>
#include <vector>

#include "modmath.h"

namespace apsu_he {

constexpr int LOOKUP_LANES = 64;
constexpr u32 LOOKUP_NONE = 0xFFFFFFFFu;                  // no point in this (row, lane); also the count of a slot that is not a bin

// one Horner step: acc <- acc x + p  (mod t)
HD u64 lookup_horner_step(u64 acc, u64 x, u64 p, const Mod &t) { return addmod(mulmod(acc, x, t), p, t.q); }

// the zero-polynomial rule: `nz` is the OR of every coefficient the lane has read; a slot that holds no polynomial has no roots
HD bool lookup_found(u64 acc, u64 nz) { return acc == 0 && nz != 0; }

// a bin's count from the index of its highest non-zero coefficient (-1: none)
HD u32 bin_count_of(int top) { return top < 0 ? LOOKUP_NONE : (u32)top; }

struct LookupWork { u32 tile, row0, nrows, pad; };

struct LookupPlan {
    std::vector<LookupWork> work;
    std::vector<u64> pts;                                 // [rows][64] points
    std::vector<u32> idx;                                 // [rows][64] part index e * F + j that the point belongs to, or LOOKUP_NONE
    size_t rows() const { return idx.size() / LOOKUP_LANES; }
};

// felts[count][F], start[count]; every start[e] + F <= n (the caller has checked it).  R: rows per work item.
inline LookupPlan lookup_plan(const u64 *felts, const u32 *start, size_t count, u32 F, size_t n, int R)
{
    const size_t tiles = (n + LOOKUP_LANES - 1) / LOOKUP_LANES;
    std::vector<u32> per_slot(tiles * LOOKUP_LANES, 0), tile_row0(tiles + 1, 0);
    for (size_t e = 0; e < count; e++)
        for (u32 j = 0; j < F; j++) per_slot[start[e] + j]++;
    for (size_t tl = 0; tl < tiles; tl++) {
        u32 rows = 0;
        for (int l = 0; l < LOOKUP_LANES; l++) rows = per_slot[tl * LOOKUP_LANES + l] > rows ? per_slot[tl * LOOKUP_LANES + l] : rows;
        tile_row0[tl + 1] = tile_row0[tl] + rows;
    }
    LookupPlan plan;
    const size_t rows = tile_row0[tiles];
    plan.pts.assign(rows * LOOKUP_LANES, 0);
    plan.idx.assign(rows * LOOKUP_LANES, LOOKUP_NONE);
    std::vector<u32> filled(tiles * LOOKUP_LANES, 0);
    for (size_t e = 0; e < count; e++)
        for (u32 j = 0; j < F; j++) {
            const size_t slot = (size_t)start[e] + j, at = ((size_t)tile_row0[slot / LOOKUP_LANES] + filled[slot]++) * LOOKUP_LANES + slot % LOOKUP_LANES;
            plan.pts[at] = felts[e * F + j];
            plan.idx[at] = (u32)(e * F + j);
        }
    for (size_t tl = 0; tl < tiles; tl++)
        for (u32 r = tile_row0[tl]; r < tile_row0[tl + 1]; r += (u32)R) {
            const u32 left = tile_row0[tl + 1] - r;
            plan.work.push_back(LookupWork{ (u32)tl, r, left < (u32)R ? left : (u32)R, 0 });
        }
    return plan;
}

}  // namespace apsu_he
