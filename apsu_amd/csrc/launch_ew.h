// Launch entry points of the element-wise kernels (kernels_ew.hip).  Contract vocabulary (canonical, RAW): device.h.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_consts.h"
#include "blake2x.h"

namespace apsu_he {

// INPUT CONTRACTS of the element-wise launchers ("contract:" lines below; tests/test_gpu_kernel_steps.py feeds every launcher exactly
// up to its contract through Engine::debug_run_step, which refuses what lies beyond it).
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
// rej: [njobs][1 + SEED_REJ_CAP] u32, zeroed once (the kernels leave the counter of every object they complete at zero); *overflow is
// set when an object has more than `cap` rejected words: that object is left incomplete with its counter standing, the others are
// complete.  A word is refused with probability (2^64 mod q) / 2^64: below 2^-27 for SEAL's primes 2^b - c, up to ~q / 2^64 otherwise.
// contract: 1 <= cap <= SEED_REJ_CAP; every max_multiple[j] well above 0 -- the fix-up redraws until a word falls below it (SEAL's
// own value exceeds 2^63 for q < 2^62); n a multiple of 8
struct SeedJob { Blake2xbSeed seed; u64 *dst; };
void launch_seed_expand(const SeedJob *jobs, int njobs, const DevLevel *lv, int L, const u64 *max_multiple, size_t n, u32 *rej, u32 cap, int *overflow,
                        hipStream_t st);
// N4: the rounding step of the querier's decryption
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

} // namespace apsu_he
