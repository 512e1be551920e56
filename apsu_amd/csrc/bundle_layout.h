// Where each coefficient of a stored BinBundle lives, as one pure function of (ps_low_degree, degree, first_chain_idx): the rule of the
// BatchedPlaintextPolyn ctor (bin_bundle.cpp:385-420) with use_ps as the receiver decides it (receiver_osn.cpp:520-522).  a_0 stays raw
// mod t; with h = ps_low_degree + 1, the coefficients a_{i*h} (i >= 1) are kept in coefficient form -- here pre-lifted and transformed at
// the high level, H = degree / h of them, slot i - 1; every other coefficient is in NTT form at pt_level, packed in ascending degree
// order.  Without Paterson-Stockmeyer (ps_low_degree == 0) every d >= 1 is of the second kind.  No HIP in here: Engine::new_bundle
// fills a Bundle from the layout, upload / finish / decode / download / load (engine_bundles.cpp) and the saved export (engine_db.cpp) read kinds, slots and runs from it and
// nowhere else; tests/test_bundle_layout_cpu.py enumerates it through the CPU emulation library against a restatement of the rule.
//
// The evaluation (engine_eval.cpp: ps_tables; engine_nks.cpp: eval_bundles_nks) relies on one consequence: the NTT-form coefficients of inner polynomial i,
// a_{i*h+1} .. a_{i*h+l} with l = ps_low_degree, start at slot i * l -- each block of h degrees holds l of them and one a_{i*h}.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace apsu_he {

enum CoeffKind { COEFF_RAW = 0, COEFF_NTT = 1, COEFF_LIFTED = 2 };      // the `kind` of Engine::download_coeff

struct BundleRun { uint32_t d0, count; int kind; uint32_t first_slot; };  // degrees d0 .. d0 + count - 1, slots first_slot .. of `kind`
struct BundleWhere { int kind; uint32_t slot; };
struct BundleLayout {
    uint32_t degree = 0;
    uint32_t h = 0;                   // ps_low_degree + 1; 0 without Paterson-Stockmeyer
    uint32_t H = 0, r = 0;            // degree / h, degree % h (bin_bundle.cpp:225-227)
    bool use_ps = false;
    int pt_level = 0;                 // chain index of the NTT-form plaintexts
    size_t ntt_count = 0, lifted_count = 0;
    std::vector<BundleRun> runs;      // d = 1 .. degree in maximal runs of one kind, ascending
    BundleWhere where(uint32_t d) const
    {
        if (d == 0) return { COEFF_RAW, 0 };
        const uint32_t below = h ? d / h : 0;                            // coefficient-form a_{i*h} with 1 <= i*h <= d
        if (h && d % h == 0) return { COEFF_LIFTED, below - 1 };
        return { COEFF_NTT, d - below - 1 };
    }
};

inline BundleLayout bundle_layout(uint32_t ps_low_degree, uint32_t degree, int first_chain_idx)
{
    const uint32_t ps = ps_low_degree;
    BundleLayout y;
    y.degree = degree;
    y.use_ps = ps > 1 && ps < degree;                                    // receiver_osn.cpp:520-522
    y.h = ps ? ps + 1 : 0;
    y.H = ps ? degree / y.h : 0;
    y.r = ps ? degree % y.h : 0;
    y.pt_level = std::min(first_chain_idx, ps ? 2 : 1);                  // bin_bundle.cpp:385-389
    if (!y.use_ps && ps && degree > ps)
        throw std::invalid_argument("ps_low_degree == 1 leaves coefficient-form plaintexts that eval() cannot multiply");
    for (uint32_t d = 1; d <= degree; d++) {
        const BundleWhere w = y.where(d);
        if (y.runs.empty() || y.runs.back().kind != w.kind) y.runs.push_back(BundleRun{ d, 0, w.kind, w.slot });
        y.runs.back().count++;
        (w.kind == COEFF_NTT ? y.ntt_count : y.lifted_count)++;
    }
    return y;
}

} // namespace apsu_he
