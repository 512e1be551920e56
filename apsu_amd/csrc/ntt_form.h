// Which form of the LDS-resident transform a launch takes, as a pure function of the ring size, the kind of launch, its number of limbs,
// the engine's latency_limbs setting and what the caller states about its moduli.  Every form gives the same bits, so the GPU parity
// tests cannot see this choice: the launch wrappers of kernels_ntt.hip dispatch from ntt_form and nothing else, and tests/test_host_logic.py
// holds it to a table through the CPU emulation library.  No HIP in here.
#pragma once
#include <cstddef>
#include "ntt_core.h"

namespace apsu_he {

// latency_limbs: 0 = always the throughput form; NTT_FORM_AUTO = the crossovers measured with tools/microbench/ntt_forms.hip
// (profiles/r06_ntt_forms_n8192.txt, _n4096.txt); any other value = a launch of at most that many limbs takes the latency form
// wherever the ring size has one, whatever its kind (tests force either form with it: APSU_HE_NTT_LATENCY_LIMBS).
constexpr size_t NTT_FORM_AUTO = ~(size_t)0;
constexpr int SPLIT_LOGN = 15;   // n = 32768: two LDS-resident half transforms around one radix-2 stage over global memory (kernels_ntt.hip)

enum NttKind { NTT_KIND_FORWARD, NTT_KIND_INVERSE, NTT_KIND_GATHER, NTT_KIND_TENSOR };
struct NttForm {
    int threads;           // per limb's workgroup; 0: no transform at this ring size
    int coeffs_per_lane;   // 16 the throughput form, 8 the latency form (twice the waves per limb, ntt_core.h plan_k)
    int min_waves;         // waves per SIMD the register budget must admit (__launch_bounds__)
    bool split;            // SPLIT_LOGN: threads .. min_waves describe the two half transforms
};

// limbs: of the launch (tensor launches: products' limbs + plain limbs).  narrow: every modulus of the launch is narrow (ntt_is_narrow).
// NTT_FORM_AUTO at n = 8192: a limb's 1024-thread workgroup wins while a CU gets at most one limb (<= 256 limbs: -3 ... -16 %) and loses
// above (+2 ... +20 %), where forward launches over narrow moduli and every gathered launch take the 8-coefficient build for 8 waves per
// SIMD instead (<= 64 VGPRs, two workgroups per CU: -4 ... -7 % and -1 ... -5 %; slower on 61-bit limbs and on every inverse).
// At n = 4096 (512 threads, registers for 7-8 waves per SIMD) the forward, gathered and tensor-on-load transforms win at every size
// (-2 ... -24 %), the plain inverse up to 1 024 limbs.
inline NttForm ntt_form(int logn, NttKind kind, size_t limbs, size_t latency_limbs, bool narrow)
{
    if (logn == SPLIT_LOGN) return { 1024, 16, 4, true };
    if (plan_passes(logn, 16) == 0) return {};
    const int n = 1 << logn;
    bool latency = false;
    if (plan_has_latency_form(logn) && latency_limbs != 0) {
        if (latency_limbs != NTT_FORM_AUTO) latency = limbs <= latency_limbs;
        else if (logn == 13) latency = limbs <= 256;
        else latency = kind != NTT_KIND_INVERSE || limbs <= 1024;
    }
    if (latency) return { n / 8, 8, 4, false };
    if (latency_limbs == NTT_FORM_AUTO && logn == 13 && (kind == NTT_KIND_GATHER || (kind == NTT_KIND_FORWARD && narrow)))
        return { 1024, 8, 8, false };
    return { n / 16 > 64 ? n / 16 : 64, 16, 4, false };
}

// ntt_lazy_input_ok bounds the tensor loader's lazy input with the throughput form's first inverse pass; the latency form's may not be larger
static_assert(plan_k(12, plan_passes(12, 16) - 1, 16) >= plan_k(12, plan_passes(12, 8) - 1, 8), "ntt_lazy_input_ok at n = 4096");
static_assert(plan_k(13, plan_passes(13, 16) - 1, 16) >= plan_k(13, plan_passes(13, 8) - 1, 8), "ntt_lazy_input_ok at n = 8192");

} // namespace apsu_he
