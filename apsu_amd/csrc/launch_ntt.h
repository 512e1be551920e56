// Launch entry points of the transforms (kernels_ntt.hip).  Contract vocabulary (canonical, RAW): device.h.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_consts.h"

namespace apsu_he {

// NTT over `count` consecutive limb polynomials of n coefficients; limb g uses
// tabs[modmap[g % period] & NTT_MAP_MASK].  An inverse transform of a limb whose map entry carries NTT_MAP_RAW (dev_consts.h) writes
// its result WITHOUT the final twist n^-1 psi^-k and without the final reduction (consumers: the unrolled BEHZ finish kernels).
// latency_limbs (NTT_FORM_AUTO, 0 or a limb count) and narrow (every modulus of the launch is a narrow data prime) choose the form of
// the transform through ntt_form (ntt_form.h).  Same bits in every form.
// contract: data canonical in both directions (the inverse's product-free butterflies add multiples of q that bound a canonical
// operand, ntt_core.h); modmap entries name tables of `tabs`, NTT_MAP_RAW in an inverse map only; out: canonical, or RAW (device.h)
// for a limb whose entry carries NTT_MAP_RAW.  n = 32768: entry m takes tables 2 m and 2 m + 1.
void launch_ntt(int logn, bool inverse, u64 *data, size_t count, const NttTable *tabs, const int *modmap,
                int period, hipStream_t st, size_t latency_limbs, bool narrow);
// forward NTT of limbs gathered from src[g] (reduced into the table's modulus on load), written to data + g*n.
// nored: the caller has checked ntt_gather_nored_ok for every (source, target) pair of the launch: no reduction on load
// contract: nored = false: a source word is ANY 64-bit word (ntt_reduce_any on load).  nored = true: every source word is below a
// max_src with ntt_gather_nored_ok(q, max_src, logn) for every target q of the map (all of them narrow: max_src + 4 logn q <= 2^64),
// and logn < SPLIT_LOGN (the split transform's first stage always reduces; the engine never asks for it there).  modmap entries
// carry no NTT_MAP_RAW (the kernel indexes `tabs` with the entry as it is).  out: canonical.
void launch_ntt_gather(int logn, const u64 *const *src, u64 *data, size_t count, const NttTable *tabs, const int *modmap, int period,
                       hipStream_t st, bool nored, size_t latency_limbs, bool narrow);
struct TensorJob { const u64 *a, *b; u64 *d; };   // a,b: [2][E][n] ext-NTT ; d: [3][E][n]
// tensor product + inverse NTT in one launch: njobs products x 3 polys x `limbs` limbs (operand polys src_ps words apart,
// output job.d[3][limbs][n], coefficient form), followed by n_plain limbs at `plain` transformed in place; modmap covers both
// (grid order: the three workgroups of one (product, limb) pair -- they read the same operand limbs -- on one XCD)
// contract: the operand limbs a, b canonical for the modulus of their limb (the fold's last word enters the transform as it is where
// ntt_lazy_input_ok holds: its bound ntt_lazy_bound_q is argued for products of canonical residues), the same modulus under the three
// map entries of one (job, limb); plain canonical; NTT_MAP_RAW per entry; out: canonical or RAW (device.h).  logn < SPLIT_LOGN.
void launch_intt_tensor(int logn, const TensorJob *jobs, int njobs, int limbs, size_t src_ps, u64 *plain, size_t n_plain,
                        const NttTable *tabs, const int *modmap, int period, hipStream_t st, size_t latency_limbs = 0);

} // namespace apsu_he
