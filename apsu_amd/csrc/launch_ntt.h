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
void launch_ntt(int logn, bool inverse, u64 *data, size_t count, const NttTable *tabs, const int *modmap,
                int period, hipStream_t st, size_t latency_limbs, bool narrow);
// forward NTT of limbs gathered from src[g] (reduced into the table's modulus on load), written to data + g*n.
// nored: the caller has checked ntt_gather_nored_ok for every (source, target) pair of the launch: no reduction on load
void launch_ntt_gather(int logn, const u64 *const *src, u64 *data, size_t count, const NttTable *tabs, const int *modmap, int period,
                       hipStream_t st, bool nored, size_t latency_limbs, bool narrow);
struct TensorJob { const u64 *a, *b; u64 *d; };   // a,b: [2][E][n] ext-NTT ; d: [3][E][n]
// tensor product + inverse NTT in one launch: njobs products x 3 polys x `limbs` limbs (operand polys src_ps words apart,
// output job.d[3][limbs][n], coefficient form), followed by n_plain limbs at `plain` transformed in place; modmap covers both
// (grid order: the three workgroups of one (product, limb) pair -- they read the same operand limbs -- on one XCD)
void launch_intt_tensor(int logn, const TensorJob *jobs, int njobs, int limbs, size_t src_ps, u64 *plain, size_t n_plain,
                        const NttTable *tabs, const int *modmap, int period, hipStream_t st, size_t latency_limbs = 0);

} // namespace apsu_he
