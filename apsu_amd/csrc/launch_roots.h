// Launch entry points of kernels_roots.hip: reading the bins of a resident BinBundle back, its ragged rows, its plaintext answer.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_consts.h"
#include "bin_roots.h"
#include "bin_split.h"

namespace apsu_he {

// reading the bins back (Engine::bundle_bins; bin_roots.h, kernels_roots.hip).  occ: the slots of the n_occ occupied bins (count >= 1);
// hits [n_occ][hstride] and found [n_occ] (zeroed beforehand): the distinct roots of each; mult [n_occ][hstride]: their multiplicities,
// written for the bins with fewer distinct roots than items only.  step: g^i, i < n; pts: the forward transform mod t of the polynomial X.
bool bin_roots_has_kernel(int logn);                 // is there a k_bin_roots for this ring size (else: the composition below)
u32 bin_roots_wg_slots(int logn);                    // workgroups of k_bin_roots the current device holds at once
// the persistent kernel: `wgs` workgroups over n_occ * grid.blocks work items, rows: [wgs][n] words of workspace
// contract (launch_bin_roots, launch_roots_gather / _scan, launch_roots_mult): t < 2^32 with (t - 1) / n <= ROOTS_MAX_COSETS cosets; poly
// residues; counts[s] = the index of the highest non-zero row of column s, 1 <= counts[s] < n for every s in occ (degree < n: one
// transform holds the polynomial); rows above a count are not read; hstride >= every count of occ; found zeroed.  At most counts[s]
// values are written to a bin's list, found[rank] counts them; nothing is written to hits or mult at or behind found[rank].
void launch_bin_roots(int logn, const u64 *poly, const u32 *occ, const u32 *counts, u32 n_occ, RootsGrid grid, u32 cosets, u32 wgs, const NttTable *tabs,
                      const int *modmap, const u32 *step, const u64 *pts, u64 g, u64 *rows, u32 *vrows, u64 *hits, u32 *found, u32 hstride, hipStream_t st);
// the plain composition, per coset c: rows[r][i] = a_i c^i of bin occ[r]; launch_ntt forward mod t; the scan (first: with the test for the root 0)
void launch_roots_gather(const u64 *poly, size_t n, const u32 *occ, const u32 *counts, u32 nrows, u64 c, Mod t, u64 *rows, hipStream_t st);
void launch_roots_scan(const u64 *rows, size_t n, u32 nrows, const u64 *pts, u64 c, Mod t, bool first, const u64 *poly, const u32 *occ, const u32 *counts,
                       u64 *hits, u32 *found, u32 hstride, hipStream_t st);
// divides the columns of poly in place
void launch_roots_mult(u64 *poly, size_t n, const u32 *occ, const u32 *counts, u32 n_occ, Mod t, const u64 *hits, const u32 *found, u32 *mult, u32 hstride,
                       hipStream_t st);
// the bins cut into k parts on the device (Engine::split_bundle; bin_split.h), behind launch_roots_mult on the same hits / found / mult.
// out: the parts' root lists in one buffer, part p at out + part_off[p] as [slot][part_stride[p]] words; counts_out [k][cstride]: part
// p's count of slot s at counts_out[p * cstride + s]; part_off, part_stride: k words each, on the device; failure: one word,
// SPLIT_NO_FAILURE beforehand.  The instance (256 / 2048 / 8192 keys of LDS, 64 / 256 / 1024 work items) follows from hstride.
// contract: k >= 1; 1 <= hstride <= SPLIT_CAP_LARGE; occ: n_occ distinct slots below cstride, 1 <= counts[s] <= hstride for each;
// hits below min(found, count) are values below 2^32; mult is read only where found < count, there below min(found, count), every word
// <= SPLIT_MULT_MAX; part_stride[p] >= split_cut(c, k, p + 1) - split_cut(c, k, p) for every occupied count c, and part p's array holds
// (largest slot of occ + 1) * part_stride[p] words.  counts_out is zeroed here, all k * cstride words.  A bin with found > count, or
// whose multiplicities do not add up to its count, lowers *failure to split_failure (atomicMin) and has nothing written: no root, and
// its counts stay 0.  For every other bin exactly the words out[part_off[p] + s * part_stride[p] + i], i < its count in part p, are
// written, and its k counts.
void launch_roots_split(const u64 *hits, const u32 *found, const u32 *mult, u32 hstride, const u32 *occ, const u32 *counts, u32 n_occ, u32 k, u64 *out,
                        const u64 *part_off, const u32 *part_stride, u32 *counts_out, u32 cstride, u64 *failure, hipStream_t st);
// the bins' polynomials as ragged rows (Engine::export_saved; bin_rows.h): out[off[s] + d] = poly[d][s], d <= counts[s], s < bins.
// off: rows_offsets' scan (bins + 1 words), tops: rows_tile_tops, both on the device; out holds off[bins] words.
// contract: rows >= 1, 1 <= bins <= n; counts[s] < rows and not LOOKUP_NONE for s < bins (rows_offsets refuses the rest), counts behind
// `bins` are not read; any words in poly (copied, no arithmetic); rows above a bin's count are read into the tile but not stored.
// Exactly the words out[0 .. off[bins]) are written.
void launch_bins_rows(const u64 *poly, size_t n, u32 rows, const u32 *counts, const u64 *off, const int *tops, u32 bins, u64 *out, hipStream_t st);
// the plaintext answer (Engine::bundles_eval_plain; bin_eval.h): out[s] = P_s(x[s]) + mask[s] mod t over poly[rows][n], counts =
// launch_bin_counts' output of the same array; mask and is_bin (1: the slot is a bin) may be null; *bad = 1 for a value >= t.  The comparison of the self-test:
// got, want [count][n]; status[0] += mismatches, status[1] = min (position << 32 | slot) of one (EVAL_NO_MISMATCH beforehand).
// contract (launch_bins_eval): rows >= 1; poly residues; counts any words: a tile walks rows min(largest count of the tile, rows - 1) .. 0
// of ALL its slots (so rows above a slot's own count are read, and must be 0 for the answer to be about the bin), a tile of LOOKUP_NONE
// alone reads nothing.  x and mask: any word; one that is not a residue raises *bad, and out of that slot is then unspecified, every
// other slot's as always.  contract (launch_eval_compare): count <= 65535 (a grid dimension); any words.
void launch_bins_eval(const u64 *poly, size_t n, u32 rows, const u32 *counts, const u64 *x, const u64 *mask, Mod t, u64 *out, unsigned char *is_bin, u32 *bad, hipStream_t st);
void launch_eval_compare(const u64 *got, const u64 *want, size_t n, u32 count, u64 *status, hipStream_t st);

} // namespace apsu_he
