// Job structs and kernel launch entry points of the query-evaluation engine.  The constant blocks the kernels read
// (DevLevel, DevKey, the transform tables and limb maps) are in dev_consts.h.  Layout of all polynomial data is SEAL's
// in-memory order [poly][limb][coeff] of uint64.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_consts.h"
#include "mac_plan.h"
#include "eval_plan.h"
#include "blake2x.h"
#include "query_side.h"
#include "bin_lookup.h"
#include "bin_merge.h"
#include "bin_roots.h"
#include "bin_rows.h"
#include "bin_eval.h"

namespace apsu_he {

// ---- launch wrappers (all asynchronous on `st`) --------------------------------------------
// INPUT CONTRACTS of the element-wise launchers ("contract:" lines below; tests/test_gpu_kernel_steps.py feeds every launcher exactly
// up to its contract through Engine::debug_run_step, which refuses what lies beyond it).
//   canonical: a word in [0, m) for the modulus m of its limb (or [0, t) for a plaintext coefficient).
//   RAW:       what an inverse transform leaves where the limb's map entry carries NTT_MAP_RAW -- no twist, no closing reduction; the
//              word w stands for the residue w n^-1 psi^-k mod m at coefficient k.  What the transform can actually leave
//              (ntt_core.h, the last inverse pass, `OUT == IO_GLOBAL && !(INV && RAW)`): for a wide modulus (not ntt_is_narrow) the
//              butterflies keep values in [0, 2^64) by csub_top alone, so ANY 64-bit word; for a narrow modulus, which runs without
//              range control, below (2^K b0 + 4 (logn - K)) m, with K the stages of the first inverse pass and b0 = 1 for a canonical
//              source or ntt_lazy_bound_q(tab) for the tensor fold's last word (ntt_lazy_input_ok) -- under 2^64 by the narrow
//              criterion, and nothing tighter is argued.  Every RAW consumer therefore takes ANY 64-bit word: its first operation on
//              the word is a Shoup product (mul_shoup / mul_shoup_lazy, modmath.h: exact for any 64-bit x, m < 2^63).
// NTT over `count` consecutive limb polynomials of n coefficients; limb g uses
// tabs[modmap[g % period] & NTT_MAP_MASK].  An inverse transform of a limb whose map entry carries NTT_MAP_RAW (dev_consts.h) writes
// its result WITHOUT the final twist n^-1 psi^-k and without the final reduction (consumers: the unrolled BEHZ finish kernels).
// latency_limbs (NTT_FORM_AUTO, 0 or a limb count) and narrow (every modulus of the launch is a narrow data prime) choose the form of
// the transform through ntt_form (ntt_form.h).  Same bits in every form.
void launch_ntt(int logn, bool inverse, u64 *data, size_t count, const NttTable *tabs, const int *modmap,
                int period, hipStream_t st, size_t latency_limbs, bool narrow);
// forward NTT of limbs gathered from src[g] (reduced into the table's modulus on load), written to data + g*n.
// nored: the caller has checked ntt_gather_nored_ok for every (source, target) pair of the launch: no reduction on load
void launch_ntt_gather(int logn, const u64 *const *src, u64 *data, size_t count, const NttTable *tabs, const int *modmap, int period,
                       hipStream_t st, bool nored, size_t latency_limbs, bool narrow);
// out = a (.) b per limb; a:[batch][polys][L][n], b:[batch][L][n] (b_batch_stride may be 0)
// contract: ct and pt canonical (one 128-bit product per word, Barrett-reduced)
void launch_dyadic_plain(const DevLevel *lv, const u64 *ct, const u64 *pt, u64 *out, int polys, size_t n, int batch,
                         size_t pt_batch_stride, hipStream_t st);
void launch_add(const DevLevel *lv, u64 *acc, const u64 *x, int polys, size_t n, int batch, hipStream_t st);
// contract (launch_add, launch_add_many, launch_sum_jobs): every word canonical -- one conditional subtraction per addition
// acc[b] += sum_{i<terms} x[b][i]   (x: [batch][terms][polys][L][n]; acc: [batch] stride acc_stride words)
void launch_add_many(const DevLevel *lv, u64 *acc, size_t acc_stride, const u64 *x, int terms, int polys, size_t n,
                     int batch, hipStream_t st);
struct SumJob { const u64 *src; u64 *dst; int terms; int pad; };
void launch_sum_jobs(const DevLevel *lv, int L, const SumJob *jobs, int polys, size_t n, int njobs, hipStream_t st);
// launch_sum_jobs: two coefficients per lane (n even, src and dst 16-byte aligned)
struct PlainJob { u64 *ct; const u64 *pt; };        // ct: c0 limbs [L][n] ; pt: n coefficients mod t
// contract (launch_add_plain, launch_lift): pt canonical mod t (m < t < 2^61: the 128-by-64 division of the scaling takes the
// shift-subtract branch only for t > 2^32), ct canonical
void launch_add_plain(const DevLevel *lv, const PlainJob *jobs, size_t n, int batch, hipStream_t st);
void launch_lift(const DevLevel *lv, const u64 *pt, u64 *out, size_t n, int batch, const unsigned char *no_lift,
                 hipStream_t st);
// drop last limb: ct c at in + c*in_stride holds `polys` polys [L][n] -> out packed [c][polys][L-1][n]
// contract (launch_modswitch, launch_modswitch_jobs): every limb canonical; L >= 2.  The dropped prime may be narrower or wider than
// the kept ones: (last + half) mod q_last is reduced into each kept prime by barrett64
void launch_modswitch(const DevLevel *lv, const u64 *in, size_t in_stride, int polys, u64 *out, size_t n, int cts,
                      hipStream_t st);
void launch_clear_bits(u64 *ct, size_t words, int bits, hipStream_t st);
struct CtJob { const u64 *src; u64 *dst; };
void launch_copy_jobs(const CtJob *jobs, size_t words, int njobs, hipStream_t st);
// copy of query source ciphertexts ([2][L][n] words each) that flags words outside [0, q_limb) in *bad (device-visible host memory)
void launch_copy_sources(const CtJob *jobs, size_t words, int njobs, const DevLevel *lv, int L, size_t n, unsigned *bad, unsigned seq, hipStream_t st);
// drop last limb of `polys` polynomials per job: src [polys][L][n] -> dst [polys][L-1][n]
void launch_modswitch_jobs(const DevLevel *lv, const CtJob *jobs, int polys, size_t n, int njobs, hipStream_t st);
void launch_fill_random(u64 *out, size_t words, u64 seed, u64 bound, hipStream_t st);
// out[i] = (the (first + i)-th 32-bit output of SEAL's Blake2xb generator under `seed`) % bound
void launch_fill_blake2xb(u64 *out, size_t words, const Blake2xbSeed &seed, u64 first, u64 bound, hipStream_t st);
// N3: c1 of seeded ciphertexts / keys = util::sample_poly_uniform under SEAL's Blake2xb generator (seal_codec.h), dst[L][n] at level lv.
// rej: [njobs][1 + 8192] u32, zeroed once (the kernels leave the counters at zero); *overflow is set when a ciphertext has more
// rejected words than the list holds (a modulus within a factor 3 of 2^64: not a SEAL modulus).
struct SeedJob { Blake2xbSeed seed; u64 *dst; };
void launch_seed_expand(const SeedJob *jobs, int njobs, const DevLevel *lv, int L, const u64 *max_multiple, size_t n, u32 *rej, int *overflow,
                        hipStream_t st);
// N1: BinBundle build (polyn_with_roots per bin, BatchEncoder scatter, monomial detection)
// INPUT CONTRACTS of the resident-database launchers ("contract:" lines from here to launch_eval_compare; tests/test_gpu_db_kernel_steps.py
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
void launch_scatter_slots(const u64 *in, const u32 *slot_map, u64 *out, size_t n, int batch, hipStream_t st);
void launch_gather_slots(const u64 *in, const u32 *slot_map, u64 *out, size_t n, int batch, hipStream_t st);
// N1: algebraize_item for `count` 16-byte items -> out[count][felts]; bpf = bits per field element, item_bits = felts * bpf
void launch_algebraize(const unsigned char *items, size_t count, u32 felts, u32 bpf, u32 item_bits, u64 *out, hipStream_t st);
// N4: item -> 128-bit block packing for PEQT, and the rounding step of the querier's decryption
void launch_pack_blocks(const u64 *values, size_t n, u32 items, u32 felts, u32 len, u64 *out, int batch, hipStream_t st);
void launch_decrypt_round(const u64 *ct, size_t ct_stride, const u64 *v, u64 q0, u64 t, u64 *out, size_t n, int batch, hipStream_t st);
// ... with the invariant noise budget's numerator: worst[b] (zeroed by the caller) = max over k of the centred |t x mod q0|
void launch_decrypt_round_budget(const u64 *ct, size_t ct_stride, const u64 *v, u64 q0, u64 t, u64 *out, size_t n, int batch, u64 *worst,
                                 hipStream_t st);
// N5: the querier's side (query_side.h has the stream layout and the value maps).  Small signed polynomials are int8 arrays.
constexpr u32 QS_FLAG_VALUE = 1;                     // k_plain_powers met a slot value >= t
// out[b * S + s][slot_map[i]] = vals[b][i]^exps[s] mod t  (BatchEncoder's pre-transform order; the inverse NTT mod t follows)
void launch_plain_powers(const u64 *vals, const u32 *slot_map, const u32 *exps, int S, Mod t, u64 *out, size_t n, int batch, u32 *flags, hipStream_t st);
void launch_sample_ternary(const Blake2xbSeed &seed, signed char *out, size_t n, hipStream_t st);
// out[c][n] = noise polynomial of object first_object + c
void launch_sample_cbd(const Blake2xbSeed &seed, u64 first_object, signed char *out, size_t n, int count, hipStream_t st);
// dst[c][j][k] = small[c][k] mod key prime j, j < limbs
void launch_small_lift(const DevKey *key, const signed char *small, u64 *dst, int limbs, size_t n, int count, hipStream_t st);
// c0 = Delta(pt) - e - v per limb, written into cts[c][0]  (cts: [count][2][L][n]; v: [count][L][n]; pt: [count][n]; e: [count][n])
void launch_enc_finish(const DevLevel *lv, const u64 *pt, const u64 *v, const signed char *e, u64 *cts, size_t n, int count, hipStream_t st);
// ksk[i][0][j] = -(ksk[i][1][j] s_j + e[i][j]) + [j == i] (p mod q_i) s_i^2  over the K key limbs, NTT domain
void launch_rlk_finish(const DevKey *key, int K, const u64 *s, const u64 *e, u64 *ksk, size_t n, hipStream_t st);
void launch_flag_monomial(const u64 *pt, size_t n, int batch, unsigned char *flag, hipStream_t st);
// BEHZ
// ct c at in + c*in_stride holds `polys` polys [L][n]; out packed [c][polys][E][n]
// contract: every limb canonical (the q limbs are copied to the output as they are)
void launch_behz_ext(const DevLevel *lv, int L, int nB, const u64 *in, size_t in_stride, int polys, u64 *out, size_t n, int cts,
                     hipStream_t st);
// mod_switch_to_next + extension in one pass (input: L + 1 limbs per polynomial at level lv + 1); false = not available for this size
// raw: `in` comes from an inverse NTT that left out its twist (NTT_MAP_RAW); needs lv[1].drop_tw / last_tw
// contract: L == nB <= 3 (behz_unrolled), else declined.  raw = false: all L + 1 limbs canonical.  raw = true: all L + 1 limbs RAW, any
// 64-bit word (the dropped limb is made canonical by one exact Shoup product, the kept ones enter a + 2q - b with a, b in [0, 2q))
bool launch_drop_behz_ext(const DevLevel *lv, int L, int nB, const u64 *in, size_t in_stride, int polys, u64 *out, size_t n, int cts,
                          hipStream_t st, bool raw = false);
// contract (launch_tensor, launch_tensor_conv, launch_tensor_sum): every operand limb canonical modulo its ext modulus (q limbs < 2^60,
// Bsk limbs < 2^61: a product is below 2^122, launch_tensor_sum folds its 128-bit sums every 8 terms = 16 products)
struct TensorJob { const u64 *a, *b; u64 *d; };   // a,b: [2][E][n] ext-NTT ; d: [3][E][n]
void launch_tensor(const DevLevel *lv, const TensorJob *jobs, size_t n, int batch, hipStream_t st);
// operands of any size: a: [sa][E][n], b: [sb][E][n] ext-NTT ; d: [sa + sb - 1][E][n]   (no key switching: products are never relinearised)
struct TensorConvJob { const u64 *a, *b; u64 *d; int sa, sb; };
void launch_tensor_conv(const DevLevel *lv, const TensorConvJob *jobs, size_t n, int njobs, hipStream_t st);
// The same for a sum of products sharing one output (eval_patstock's sum over i): a, b: [terms][2][E][n];
// dq: [terms][3][L][n] per-term q limbs; bs: [3][nBsk][n] Bsk limbs summed over the terms
struct TensorSumJob { const u64 *a, *b; u64 *dq, *bs; int terms; int pad; };
// e0: first ext limb handled (0: everything; L: only the Bsk sums, the per-term q limbs being formed by launch_intt_tensor)
void launch_tensor_sum(const DevLevel *lv, int E, const TensorSumJob *jobs, size_t n, int njobs, int e0, hipStream_t st);
// tensor product + inverse NTT in one launch: njobs products x 3 polys x `limbs` limbs (operand polys src_ps words apart,
// output job.d[3][limbs][n], coefficient form), followed by n_plain limbs at `plain` transformed in place; modmap covers both
// (grid order: the three workgroups of one (product, limb) pair -- they read the same operand limbs -- on one XCD)
void launch_intt_tensor(int logn, const TensorJob *jobs, int njobs, int limbs, size_t src_ps, u64 *plain, size_t n_plain,
                        const NttTable *tabs, const int *modmap, int period, hipStream_t st, size_t latency_limbs = 0);
struct FinishSumJob { const u64 *dq, *bs; u64 *out; int terms; int pad; };   // out: [3][L][n] = sum of the finished terms
// contract (launch_behz_finish_sum, launch_behz_finish): for L == nB <= 3 (behz_unrolled) dq / bs / d are RAW, any 64-bit word (the twist
// is part of fin_q / fin_b), and ONLY RAW; every other level takes canonical limbs.  An accumulated-into `out` is canonical.
// launch_behz_finish_sum adds the per-term canonical residues of a q limb as plain integers: terms * q_widest < 2^63 (plan_eval,
// p.summed; the kernels themselves need terms * q_j < 2^64)
void launch_behz_finish_sum(const DevLevel *lv, int L, int nB, const FinishSumJob *jobs, size_t n, int njobs, hipStream_t st);
// finish: out[3][L][n] (+)= sum over `terms` consecutive products d[term][3][E][n] (coeff form)
struct FinishJob { const u64 *d; u64 *out; int terms; int pad; };
void launch_behz_finish(const DevLevel *lv, int L, int nB, const FinishJob *jobs, bool accumulate, size_t n, int njobs, hipStream_t st);
// key switching
// contract: tdec limb (I, J) canonical modulo m_I (the key moduli of this level, then the special prime), rk canonical: at most DMAXL
// products below 2^120 per 128-bit sum
void launch_ks_inner(const DevKey *key, int L, const u64 *tdec, const u64 *rk, u64 *acc, size_t n, int batch,
                     hipStream_t st);
// raw: acc comes from an inverse NTT that left out its twist (L <= 4; needs key->md_tw / p_tw)
// contract: ct canonical.  raw = false: acc canonical (the special limb below p).  raw = true: all L + 1 limbs of acc RAW, any 64-bit
// word; L <= 4.  ext / n_ext: only for L == nB <= 3 (the caller checks)
void launch_ks_moddown(const DevKey *key, int L, const u64 *acc, u64 *ct, size_t ct_stride, size_t n, int batch,
                       hipStream_t st, const DevLevel *lv = nullptr, u64 *ext = nullptr, int n_ext = 0, bool raw = false);
// k_mac over njobs MacJobs (mac_core.h) in the form (kara: three products; packed: bit-packed plaintexts) and on the grid of a MacPlan (mac_plan.h)
void launch_mac(const DevLevel *lv, int nlimbs, const MacJob *jobs, size_t n, int njobs, hipStream_t st, bool kara, bool packed, MacGrid grid);
// single products on one limb: out[0][k] = a[k] * pw[limb][k], out[out_poly_stride + k] = a[k] * pw[pw_poly_stride + limb n + k]  (mod q_limb);
// pt: the plaintext's slot as k_mac takes it (dense: [L][n] words; packed: the bit-packed slot, rows per DevLevel::mac_row_off)
void launch_term_product(const DevLevel *lv, const TermJob *jobs, size_t njobs, size_t n, int limb, u32 pw_poly_stride, u32 out_poly_stride,
                         bool packed, hipStream_t st);
// dense [slots][L][n] u64 <-> bit-packed [slots][slot_bytes] (rows per DevLevel::mac_bits / mac_row_off of `lv`)
void launch_pack_rows(const DevLevel *lv, int L, const u64 *dense, void *packed, size_t slot_bytes, size_t n, size_t slots, hipStream_t st);
void launch_unpack_rows(const DevLevel *lv, int L, const void *packed, size_t slot_bytes, u64 *dense, size_t n, size_t slots, hipStream_t st);
// Fused tail of eval / eval_patstock (bin_bundle.cpp:159-171, 345-357): (c0,c1) (+ optional exact addends) + Delta*a0 +
// Delta*mask, drop limbs down to the last level, clear the irrelevant bits, write the 2n-word result.
// contract: ct, add1, add2 canonical at level lvl; a0 and mask canonical mod t; with a key, ks_acc RAW (any 64-bit word) and lvl + 1 <= 4
struct EpiJob { const u64 *ct; const u64 *add1; const u64 *add2; const u64 *a0; const u64 *mask; u64 *out;
                const u64 *ks_acc = nullptr; };   // round 6: RAW key-switch sums [2][L+1][n] whose mod-down the epilogue performs (launch_eval_epilogue with a key)
void launch_eval_epilogue(const DevLevel *levels, int lvl, const EpiJob *jobs, size_t ct_poly_stride, int clear_bits, size_t n,
                          int njobs, hipStream_t st, const DevKey *key = nullptr);
// i = 0 block of eval_patstock when exactly one limb is dropped (bin_bundle.cpp:314-324, note N1):
// acc[p][m] += (S[p][m] + terms*half - sum_t ((V[t][p] + half) mod q_last)) * q_last^-1  mod q_m
struct I0Job { const u64 *s; const u64 *v; u64 *acc; int terms; int store; };   // s:[2][L-1][n] v:[terms][2][n] acc:[2][L-1][n] (store: = instead of +=)
// raw: s and v come from an inverse NTT that left out its twist (needs lv_low->drop_tw / last_tw)
// contract: L >= 2 at lv_low; (terms + 1) * q_last < 2^64 (plan_eval, p.i0_fast); acc canonical unless stored.  raw = false: s and v
// canonical.  raw = true: s and v RAW, any 64-bit word
void launch_i0_finish(const DevLevel *lv_low, const I0Job *jobs, size_t n, int njobs, hipStream_t st, bool raw = false);

} // namespace apsu_he
