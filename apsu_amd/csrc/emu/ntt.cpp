// CPU emulation, transforms and reductions (ntt_core.h; the workgroup driver: ntt_driver.h).  Held to an integer model by
// tests/test_ntt_step_model_cpu.py and tests/test_host_logic.py.
#include "emu_common.h"
#include "ntt_driver.h"

using namespace apsu_he;

extern "C" {

// One limb with the product's tables for modulus q (n = 2^logn) as k_ntt / k_ntt_gather run it, with the template arguments the kernels
// pass to ntt_body (tests/test_ntt_step_model_cpu.py): coeffs = coefficients per work item; red 0 = in place on data; 1 / 2 = the forward
// transform of `src` (another modulus' residues reduced on load / any words taken as they are: k_ntt_gather with nored 0 / 1) written to
// data; raw = the inverse transform without its twist and closing reduction (NTT_MAP_RAW).  Refused: red with an inverse transform or
// without a source, raw with a forward one, red 2 for a modulus that is not narrow (the kernel reduces there).
int emu_ntt_limb_ex(int logn, int inverse, uint64_t q, const uint64_t *src, uint64_t *data, int threads, int coeffs, int red, int raw)
{
    return guarded([&]() -> int {
        emu_check_coeffs(logn, coeffs);
        if (red < 0 || red > 2 || (red && (inverse || !src)) || (raw && !inverse)) throw std::invalid_argument("red is for a forward transform with a source, raw for an inverse one");
        const EmuTables et(logn, q);
        const NttTable &tab = et.tab;
        if (red == 2 && !tab.narrow) throw std::invalid_argument("an unreduced gather needs a narrow modulus");
        emu_with_shape(logn, coeffs, [&](auto ln, auto c) {
            emu_with_mode(tab, [&](auto mode) {
                constexpr int LOGN = decltype(ln)::value, C = decltype(c)::value, MODE = decltype(mode)::value;
                // the kernels' wave-uniform branches: k_ntt (the inverse stages its limb: SrcStaged; RAW from the map entry), k_ntt_gather
                if (inverse && raw) emu_ntt_body<LOGN, true, MODE, 0, true, SrcStaged, C>(data, tab, threads);
                else if (inverse) emu_ntt_body<LOGN, true, MODE, 0, false, SrcStaged, C>(data, tab, threads);
                else if (red == 0) emu_ntt_body<LOGN, false, MODE, 0, false, SrcPlain, C>(data, tab, threads);
                else if (red == 1) emu_ntt_body<LOGN, false, MODE, 1, false, SrcPlain, C>(data, tab, threads, src);
                else if constexpr (MODE == NTT_NARROW) emu_ntt_body<LOGN, false, MODE, 2, false, SrcPlain, C>(data, tab, threads, src);
            });
        });
        return 0;
    });
}
// the transform in place: coeffs = 16, or 8 where the ring size has the latency form (logn 12 and 13)
int emu_ntt_limb_c(int logn, int inverse, uint64_t q, uint64_t *data, int threads, int coeffs)
{
    return emu_ntt_limb_ex(logn, inverse, q, nullptr, data, threads, coeffs, 0, 0);
}
int emu_ntt_limb(int logn, int inverse, uint64_t q, uint64_t *data, int threads) { return emu_ntt_limb_c(logn, inverse, q, data, threads, 16); }

// INTT(x0*y0 (+ x1*y1)) of one limb through the fused loader (k_intt_tensor: SrcTensor); x1 = y1 = NULL for a single product.
// coeffs | 0x100: the products enter as the fold's last word (< 4q) where the engine would take them so (ntt_lazy_input_ok), -3 where it
// would not; coeffs | 0x200: the limb's map entry carries NTT_MAP_RAW.  Returns -2 when the modulus does not admit the 128-bit fold
// reduction (the engine then keeps the separate tensor kernel).
int emu_intt_tensor_limb_c(int logn, uint64_t q, const uint64_t *x0, const uint64_t *y0, const uint64_t *x1, const uint64_t *y1,
                           uint64_t *out, int threads, int coeffs)
{
    return guarded([&]() -> int {
        emu_check_coeffs(logn, coeffs & 0xff);
        const EmuTables et(logn, q);
        const NttTable &tab = et.tab;
        if (!ntt_fold128_ok(tab.fold_k, tab.fold_c)) return -2;
        const bool lazy = (coeffs & 0x100) != 0, raw = (coeffs & 0x200) != 0;
        if (lazy && !ntt_lazy_input_ok(tab, logn)) return -3;
        const SrcTensor ops{ x0, y0, x1, y1, lazy };
        emu_with_shape(logn, coeffs & 0xff, [&](auto ln, auto c) {
            emu_with_mode(tab, [&](auto mode) {
                constexpr int LOGN = decltype(ln)::value, C = decltype(c)::value, MODE = decltype(mode)::value;
                if (raw) emu_ntt_body<LOGN, true, MODE, 0, true, SrcTensor, C>(out, tab, threads, nullptr, ops);
                else emu_ntt_body<LOGN, true, MODE, 0, false, SrcTensor, C>(out, tab, threads, nullptr, ops);
            });
        });
        return 0;
    });
}
int emu_intt_tensor_limb(int logn, uint64_t q, const uint64_t *x0, const uint64_t *y0, const uint64_t *x1, const uint64_t *y1,
                         uint64_t *out, int threads)
{
    return emu_intt_tensor_limb_c(logn, q, x0, y0, x1, y1, out, threads, 16);
}

// ntt_reduce128_lazy on explicit (hi, lo) pairs, then ntt_lazy_bound_q and ntt_lazy_input_ok(logn) in out[count], out[count + 1];
// returns fold_k, 0 when the modulus does not admit the fold
int emu_reduce128_lazy(uint64_t q, int logn, const uint64_t *hi, const uint64_t *lo, uint64_t *out, int count)
{
    const NttTable tab = make_ntt_table(q, logn);
    if (!ntt_fold128_ok(tab.fold_k, tab.fold_c)) return 0;
    for (int i = 0; i < count; i++) out[i] = ntt_reduce128_lazy(hi[i], lo[i], tab);
    out[count] = ntt_lazy_bound_q(tab);
    out[count + 1] = plan_passes(logn, 16) ? (u64)ntt_lazy_input_ok(tab, logn) : 0;
    return (int)tab.fold_k;
}

// ntt_reduce128_fold on explicit (hi, lo) pairs; returns 0 when the modulus does not admit it
int emu_reduce128(uint64_t q, const uint64_t *hi, const uint64_t *lo, uint64_t *out, int count)
{
    const NttTable tab = make_ntt_table(q, 0);                  // (the reductions do not look at the transform's depth)
    if (!ntt_fold128_ok(tab.fold_k, tab.fold_c)) return 0;
    for (int i = 0; i < count; i++) out[i] = ntt_reduce128_fold(hi[i], lo[i], tab);
    return (int)tab.fold_k;
}

// ntt_reduce_any (the fold / Barrett final reduction of the NTT kernels) on explicit values; returns fold_k
int emu_reduce_any(uint64_t q, const uint64_t *x, uint64_t *out, int count)
{
    const NttTable tab = make_ntt_table(q, 0);
    for (int i = 0; i < count; i++) out[i] = ntt_reduce_any(x[i], tab);
    return (int)tab.fold_k;
}

// make_ntt_table for modulus q and `logn` stages: out = q, ninv, ninv_q, r1, r0, narrow, fold_k, fold_c, wide_d4.  with_tables = 1: the
// form that takes the modulus' tables (q = 1 mod 2^(logn+1)); 0: the modulus-only form (ninv = ninv_q = 0)
int emu_ntt_table(uint64_t q, int logn, int with_tables, uint64_t *out)
{
    return guarded([&]() -> int {
        const NttTable tab = with_tables ? make_ntt_table(HeParams::Create((size_t)1 << logn, { q }, 65537 < q ? 65537 : 3).ntt[0], logn, nullptr, nullptr, nullptr)
                                         : make_ntt_table(q, logn);
        const u64 v[9] = { tab.q, tab.ninv, tab.ninv_q, tab.r1, tab.r0, (u64)tab.narrow, tab.fold_k, tab.fold_c, tab.wide_d4 };
        for (int i = 0; i < 9; i++) out[i] = v[i];
        return 0;
    });
}

} // extern "C"
