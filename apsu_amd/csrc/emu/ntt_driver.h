// One workgroup of the LDS-resident transform on the CPU (host only; ntt.cpp and roots.cpp): ntt_wg.h's ntt_body as the library's kernels
// instantiate it (the branch without twiddle prefetch), with the same ntt_pass template arguments in the same order, the threads stepped
// one after the other between the points where the kernel synchronises.  The in-place global reads and writes of a pass touch disjoint
// sets of C coefficients per work item, so that stepping is equivalent to the barrier-separated parallel execution.
#pragma once
#include <stdexcept>
#include <type_traits>
#include <vector>

#include "dev_consts.h"

namespace apsu_he {

// pass PASS (in execution order) and the ones behind it
template <int LOGN, bool INV, int MODE, int RED, bool RAW, class SRC, int C, int PASS = 0>
void emu_ntt_passes(u64 *lds, u64 *p, const NttTable &tab, int T, const u64 *src, const SRC &operands)
{
    if constexpr (PASS < plan_passes(LOGN, C)) {
        if constexpr (PASS > 0) {                                    // (RAW only concerns the pass that leaves the inverse transform, the last one)
            for (int tid = 0; tid < T; tid++) ntt_pass<LOGN, INV, MODE, PASS, 0, RAW, SrcPlain, false, TwInline, NoHook, C>(lds, p, tid, T, tab);
        } else if constexpr (RED != 0) {                             // forward only: pass 0 just reads, from the gathered limb
            for (int tid = 0; tid < T; tid++) ntt_pass<LOGN, INV, MODE, 0, RED, false, SrcPlain, false, TwInline, NoHook, C>(lds, const_cast<u64 *>(src), tid, T, tab);
        } else if constexpr (!std::is_same<SRC, SrcPlain>::value) {  // every thread's coalesced sweep into the LDS image, the first pass from there
            for (int tid = 0; tid < T; tid++)
                for (int e = 2 * tid; e < (1 << LOGN); e += 2 * T) *reinterpret_cast<u64x2 *>(lds + lds_slot(e)) = src_load2(operands, p, e, tab);
            // (the source rides along: its input bound sets the constant of the first pass's multiplication-free butterflies)
            for (int tid = 0; tid < T; tid++) ntt_pass<LOGN, INV, MODE, 0, 0, false, SRC, true, TwInline, NoHook, C>(lds, p, tid, T, tab, operands);
        } else
            for (int tid = 0; tid < T; tid++) ntt_pass<LOGN, INV, MODE, 0, 0, false, SrcPlain, false, TwInline, NoHook, C>(lds, p, tid, T, tab);
        emu_ntt_passes<LOGN, INV, MODE, RED, RAW, SRC, C, PASS + 1>(lds, p, tab, T, src, operands);
    }
}

// ntt_body's template parameters without the device-only ones (T is a run-time argument here): one limb at p, T threads
template <int LOGN, bool INV, int MODE, int RED = 0, bool RAW = false, class SRC = SrcPlain, int C = 16>
void emu_ntt_body(u64 *p, const NttTable &tab, int T, const u64 *src = nullptr, const SRC &operands = SRC())
{
    constexpr int N = 1 << LOGN;
    static_assert(plan_passes(LOGN, C) > 0, "no pass schedule for this ring size and coefficients per lane");
    std::vector<u64> lds(lds_slots(N));
    emu_ntt_passes<LOGN, INV, MODE, RED, RAW, SRC, C>(lds.data(), p, tab, T, src, operands);
    if constexpr (!INV) for (int e = 0; e < N; e++) p[e] = ntt_fwd_finish<MODE>(lds[lds_slot(e)], tab);
}

// the product's transform tables for one modulus
struct EmuTables {
    std::vector<TwPair> fwd, dit, sc;
    NttTable tab;
    EmuTables(int logn, u64 q)
    {
        const size_t n = (size_t)1 << logn;
        const HeParams hp = HeParams::Create(n, { q }, 65537 < q ? 65537 : 3);   // (the plain modulus does not enter the tables: any value below q)
        const NttTablesHost &t = hp.ntt[0];
        fwd.resize(n); dit.resize(n); sc.resize(n);
        for (size_t k = 0; k < n; k++) {
            fwd[k] = { t.fwd[k], t.fwd_q[k] };
            dit[k] = { t.dit[k], t.dit_q[k] }; sc[k] = { t.scale[k], t.scale_q[k] };
        }
        tab = make_ntt_table(t, logn, fwd.data(), dit.data(), sc.data());
    }
};

// fn(MODE) for the table's modulus, as the kernels' wave-uniform branches pick it
template <class F> void emu_with_mode(const NttTable &tab, F &&fn)
{
    if (tab.narrow) fn(std::integral_constant<int, NTT_NARROW>());
    else if (tab.wide_d4) fn(std::integral_constant<int, NTT_WIDE_NEAR>());
    else fn(std::integral_constant<int, NTT_WIDE>());
}

// coeffs = coefficients per work item: 16, or 8 where the ring size has the latency form (ntt_core.h plan_k)
inline void emu_check_coeffs(int logn, int coeffs)
{
    if (coeffs != 16 && !(coeffs == 8 && plan_has_latency_form(logn))) throw std::invalid_argument("no pass schedule for this ring size and coefficients per work item");
}
// fn(LOGN, C) for a checked (logn, coeffs)
template <class F> void emu_with_shape(int logn, int coeffs, F &&fn)
{
    using C8 = std::integral_constant<int, 8>;
    using C16 = std::integral_constant<int, 16>;
    if (coeffs == 8) return logn == 13 ? fn(std::integral_constant<int, 13>(), C8()) : fn(std::integral_constant<int, 12>(), C8());
    switch (logn) {
        case 14: return fn(std::integral_constant<int, 14>(), C16());
        case 13: return fn(std::integral_constant<int, 13>(), C16());
        case 12: return fn(std::integral_constant<int, 12>(), C16());
        case 11: return fn(std::integral_constant<int, 11>(), C16());
        case 10: return fn(std::integral_constant<int, 10>(), C16());
        case 8: return fn(std::integral_constant<int, 8>(), C16());
        case 6: return fn(std::integral_constant<int, 6>(), C16());
        default: throw std::invalid_argument("unsupported logn");
    }
}

} // namespace apsu_he
