// Launch entry points of the resident-database kernels (kernels_db.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "dev_consts.h"
#include "bin_lookup.h"

namespace apsu_he {

// N1: BinBundle build (polyn_with_roots per bin, BatchEncoder scatter; the monomial detection is launch_flag_monomial, launch_ew.h)
// INPUT CONTRACTS of the resident-database launchers ("contract:" lines here and in launch_roots.h; tests/test_gpu_db_kernel_steps.py
// feeds every one exactly up to its contract through Engine::debug_run_step, which refuses what lies beyond it).  All of them work on
// poly[rows][n] words, column s = the polynomial of bin (slot) s mod t, coefficient d in row d; "residue" = a word in [0, t), t < 2^60.
// contract: 1 <= bins <= n; counts[s] <= stride and <= max_deg; roots[s][r] a residue for r < counts[s] (the words behind a bin's count
// are not read).  poly holds max_deg + 1 rows, all written (zeroed first).  max_deg / 64 + 1 register slots choose the instance: 1, 2, 4, 8,
// 16, 24, 32, 48, 64, 96, 128, and beyond 128 slots (max_deg >= 8192) the serial kernel.
void launch_polyn_with_roots(const u64 *roots, const u32 *counts, u32 bins, u32 stride, u32 max_deg, Mod t, u64 *poly, size_t n,
                             hipStream_t st);
// BinBundle update (Engine::update_bundle): limb 0 of stored plaintext slots, the un-lift, the per-bin polynomial update on the
// columns of poly[rows][n] (status: two words, both ~0 beforehand), the degree of the batched polynomial (out: one word, 0 beforehand)
void launch_limb0_rows(const DevLevel *lv, int L, const void *src, size_t slot_bytes, bool packed, u64 *out, size_t n, size_t count, hipStream_t st);
// contract (launch_unlift): q0 > 2 t; every word is a value below t or a lifted one in [q0 - t, q0) (bin_unlift; anything between the two
// ranges has no meaning and would wrap)
void launch_unlift(u64 *x, size_t words, u64 t, u64 q0, hipStream_t st);
// contract (launch_bins_update): rows >= 1; touched[w] < n, no bin named twice (one wave per entry, in place); ins / rem are indexed by
// the BIN: ins[s * ins_stride + r], r < ins_counts[s] <= ins_stride, residues (likewise rem; a null counts array = no such list).  A
// touched column holds residues in all its rows; its count c is the index of its highest non-zero row, and c - rem_counts[s] + ins_counts[s] <=
// rows - 1 (the host sizes the array: the kernels do not check, and the serial one would write behind it; the engine's rows = degree +
// most insertions + 1 is on the safe side of this).  Columns not named are neither read
// nor written.  (rows + 63) / 64 register slots choose the instance as in the build; above 128 slots (rows > 8192) the serial kernel.
// For 48 slots and more the removal is a loop over single slots, up to 32 the recursion bins_remove_slots.
// Outcome per touched bin: the updated column, zero above the new count, and counts_out[w] = the new count; OR the zero polynomial:
// status[1] = min(bin), nothing written; OR removal r leaves a remainder: status[0] = min(bin << 32 | r), counts_out[w] not written, the
// column untouched by the wave-per-bin instances and UNSPECIFIED after the serial one (which divides in place; the engine discards the
// array on either status).
void launch_bins_update(const u32 *touched, u32 n_touched, const u64 *ins, const u32 *ins_counts, u32 ins_stride, const u64 *rem,
                        const u32 *rem_counts, u32 rem_stride, Mod t, u64 *poly, size_t n, u32 rows, u32 *counts_out, u64 *status, hipStream_t st);
// contract (launch_poly_degree, launch_bin_counts): rows >= 1; any words (tested for zero only).  poly_degree: max over the slots of the
// highest non-zero row, row 0 not counted (*out 0 beforehand: the result is >= what it held)
void launch_poly_degree(const u64 *poly, size_t n, u32 rows, u64 *out, hipStream_t st);
// find and place (Engine::lookup_bundles; bin_lookup.h): per-slot counts of poly[rows][n] (LOOKUP_NONE: the zero polynomial), and the
// root test of the planned points (lookup_plan with LOOKUP_R rows per work item) -> flags[part], one byte each
constexpr int LOOKUP_R = 8;                          // points per lane of k_bins_lookup (resource report: profiles/r10_bundle_lookup.txt)
void launch_bin_counts(const u64 *poly, size_t n, u32 rows, u32 *counts, hipStream_t st);
// contract (launch_bins_lookup): poly holds degree + 1 rows of residues, ALL read by every work item (rows above a slot's count must be
// 0 for the answer to be about the bin); pts residues in every cell of a row a work item names (cells without a point are evaluated
// too); work[w]: tile < ceil(n / 64), 1 <= nrows <= LOOKUP_R, row0 + nrows <= the plan's rows; idx: LOOKUP_NONE or a part below the size
// of flags, no part twice.  flags[part] is written for exactly the parts named; the others keep their bytes.
void launch_bins_lookup(const LookupWork *work, u32 n_work, const u64 *pts, const u32 *idx, Mod t, const u64 *poly, size_t n, u32 degree,
                        unsigned char *flags, hipStream_t st);
// merge (Engine::merge_bundles; bin_merge.h): C[rows][n] = the per-slot products of A's and B's polynomials mod t, rows = the largest
// count of A + that of B + 1.  topsA / topsB: per tile of 64 slots the largest count, -1 for none (merge_tile_tops); A and B hold at
// least top + 1 rows for every tile.
// contract: rows >= 1 (any number: C is the product cut off at `rows` rows, zero from topA + topB + 1 on); -1 <= tops[tile] < the rows its
// array holds; rows 0 .. top of a tile are residues; rows above a tile's top are NOT read and may hold anything -- so an operand is, per
// tile, the polynomial of its rows 0 .. top.  The lazy sums are exact for residues only (bin_merge.h: merge_fold_exact).
void launch_bins_merge(const u64 *A, const int *topsA, const u64 *B, const int *topsB, Mod t, u64 *C, size_t n, u32 rows, hipStream_t st);
void launch_scatter_slots(const u64 *in, const u32 *slot_map, u64 *out, size_t n, int batch, hipStream_t st);
void launch_gather_slots(const u64 *in, const u32 *slot_map, u64 *out, size_t n, int batch, hipStream_t st);
// N1: algebraize_item for `count` 16-byte items -> out[count][felts]; bpf = bits per field element, item_bits = felts * bpf
void launch_algebraize(const unsigned char *items, size_t count, u32 felts, u32 bpf, u32 item_bits, u64 *out, hipStream_t st);
// N1, a whole database from its entries (Engine::build_from_entries; bulk_place.h): the root lists of target BinBundle k of one bundle index.
// contract (launch_entries_scatter): items 16-byte aligned, [offsets[locations] - offsets[0]][16] bytes; offsets [locations + 1] ascending;
// kstart [locations], any words; 1 <= F <= SCATTER_MAX_F, 1 <= bpf <= 64, (F - 1) bpf < 128; cap >= 1; every location's chunk
// bulk_chunk(kstart[l], c_l, k, cap).len <= stride < 2^30; locations F <= n_counts.  roots [bins][stride] with bins >= locations F:
// words r < len of bins l F .. l F + F - 1 are written, no other; counts [n_counts]: all written, 0 from locations F on.
// blocks: workgroups per location, 0 = scatter_blocks' choice.
void launch_entries_scatter(const void *items, const u64 *offsets, const u32 *kstart, u32 locations, u32 F, u32 bpf, u32 item_bits, u32 cap, u32 k,
                            u32 stride, u64 *roots, u32 *counts, u32 n_counts, u32 blocks, hipStream_t st);
// N4: item -> 128-bit block packing for PEQT
void launch_pack_blocks(const u64 *values, size_t n, u32 items, u32 felts, u32 len, u64 *out, int batch, hipStream_t st);

} // namespace apsu_he
