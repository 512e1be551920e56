// Launch entry points of BFV multiply (BEHZ), the key switch and the evaluation's tail (kernels_behz.hip).
// Contract vocabulary (canonical, RAW): device.h.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_consts.h"
#include "launch_ntt.h"                  // TensorJob

namespace apsu_he {

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
void launch_tensor(const DevLevel *lv, const TensorJob *jobs, size_t n, int batch, hipStream_t st);
// operands of any size: a: [sa][E][n], b: [sb][E][n] ext-NTT ; d: [sa + sb - 1][E][n]   (no key switching: products are never relinearised)
struct TensorConvJob { const u64 *a, *b; u64 *d; int sa, sb; };
void launch_tensor_conv(const DevLevel *lv, const TensorConvJob *jobs, size_t n, int njobs, hipStream_t st);
// The same for a sum of products sharing one output (eval_patstock's sum over i): a, b: [terms][2][E][n];
// dq: [terms][3][L][n] per-term q limbs; bs: [3][nBsk][n] Bsk limbs summed over the terms
struct TensorSumJob { const u64 *a, *b; u64 *dq, *bs; int terms; int pad; };
// e0: first ext limb handled (0: everything; L: only the Bsk sums, the per-term q limbs being formed by launch_intt_tensor)
void launch_tensor_sum(const DevLevel *lv, int E, const TensorSumJob *jobs, size_t n, int njobs, int e0, hipStream_t st);
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
