// Launch entry points of kernels_roots.hip: reading the bins of a resident BinBundle back, its ragged rows, its plaintext answer.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_consts.h"
#include "bin_roots.h"

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
