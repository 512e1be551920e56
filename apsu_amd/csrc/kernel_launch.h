// What the device translation units (kernels_*.hip) share; private to them.
// Hand-written gfx950 kernels of the homomorphic query-evaluation engine.
// Each kernel names the seal::Evaluator step it replaces and the reference call sites.
// Conventions: 64-lane waves, 256-thread workgroups for coefficient-parallel kernels (one thread
// per coefficient index, consecutive lanes on consecutive coefficients -> 512 B per wave access),
// level constants read through wave-uniform loads.  No MFMA: the work is modular-integer
// butterflies and dyadic products (BASELINE.json north_star).
#pragma once
#include <hip/hip_runtime.h>
#include "dev_consts.h"

namespace apsu_he {

#define KERNEL_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) throw_hip(e_, __FILE__, __LINE__); } while (0)
void throw_hip(hipError_t e, const char *file, int line);

// grid of the coefficient-parallel kernels: EW_T lanes along the coefficients, `batch` along y
static inline dim3 ew_grid(size_t n, int batch) { return dim3((unsigned)((n + EW_T - 1) / EW_T), (unsigned)batch); }

// Delta(m) of SEAL's BFV scaling (App. B7): round(m*Q/t) = m*floor(Q/t) + fix in RNS, fix = floor((m*(Q mod t) + floor((t+1)/2)) / t).
// Shared by add_plain (k_add_plain), the querier's encryption (k_enc_finish) and the evaluation's fused tail (k_eval_epilogue).
__device__ __forceinline__ u64 scaled_plain(const DevLevel *__restrict__ lv, u64 m, u64 fix, int j)
{
    u128p s = mul128(m, lv->coeff_div_plain[j]);
    add128(s, u128p{ fix, 0 });
    return barrett128(s, lv->q[j]);
}
__device__ __forceinline__ u64 plain_fix(const DevLevel *__restrict__ lv, u64 m)
{
    // floor((m * (Q mod t) + floor((t+1)/2)) / t), exact (m < t < 2^61)
    u128p num = mul128(m, lv->q_mod_t);
    add128(num, u128p{ lv->threshold, 0 });
    const u64 t = lv->t;
    if (num.hi == 0) return num.lo / t;
    u64 rem = num.hi % t, lo = num.lo, fix = 0;
    for (int i = 0; i < 64; i++) {
        rem = (rem << 1) | (lo >> 63);
        lo <<= 1;
        fix <<= 1;
        if (rem >= t) { rem -= t; fix |= 1; }
    }
    return fix;
}

} // namespace apsu_he
