// One pure function from the streams of a multiply-accumulate launch to the launch: the jobs, the profile units, the form
// (three products or four, packed rows or dense) and the grid.  No HIP: the engine launches what it returns (Engine::d_mac), and the
// CPU tier enumerates it (emu/mac.cpp, tests/test_mac_core_cpu.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "mac_core.h"

namespace apsu_he {

// one stream of a multiply-accumulate; mac_plan packs streams that share the powers and the term count into MacJobs of up to MAC_G streams
struct MacStream { const u64 *pt; const u64 *pw; u64 *out; u32 cnt, pt_stride, pw_stride, pw_poly_stride, out_poly_stride, limb0, nl; u32 packed = 0; };

// grid of k_mac: gx blocks of EW_T lanes along the coefficients; limb slowest (k_mac) unless the jobs do not fit grid dimension y
struct MacGrid { unsigned gx; int limb_slow; };
inline MacGrid mac_grid(size_t n, size_t njobs) { return MacGrid{ (unsigned)((n / MAC_C + EW_T - 1) / EW_T), njobs <= 65535u ? 1 : 0 }; }

// k_pack_rows / k_unpack_rows take (slot, limb) from grid dimension y: slots * L rows is all a launch can address.  Every caller of
// launch_pack_rows / launch_unpack_rows asks this first (a BinBundle of 8192 coefficients at 8 limbs would pass it)
constexpr size_t PACK_ROWS_GRID_Y = 65535;
inline void pack_rows_grid_check(size_t slots, int L)
{
    if (L < 1 || slots > PACK_ROWS_GRID_Y / (size_t)L)
        throw std::invalid_argument("pack_rows / unpack_rows: " + std::to_string(slots) + " slots of " + std::to_string(L) +
                                    " limbs exceed the 65535 rows of one launch (grid dimension y)");
}

struct MacPlan {
    std::vector<MacJob> jobs;
    int nlimbs = 0;                  // limbs of the level (grid extent; a job handles limb0 .. limb0 + nl - 1 of them)
    size_t n = 0;                    // coefficients per limb
    uint64_t units = 0;              // P_MAC's profile unit: BITS of rows per coefficient index (64 per dense limb, mac_bits per packed one, times terms and streams)
    uint32_t mean_cnt = 0;           // mean number of terms per (stream, limb) chain
    bool kara = false, packed = false;
    MacGrid grid{ 0, 1 };
};

// q: the primes of the level, nlimbs of them.  kara_switch: EngineSwitches::mac_kara (0 / 1: the three-product form forced off / on
// wherever every prime admits it, mac_kara_usable; < 0: by chain length -- it pays for long chains only: macbench,
// profiles/r04_mac_kara.txt, has it 1.2 % slower at 44 terms per chain (16M-4096) and 2 % faster at 150 (256M-4096 has 310)).
inline MacPlan mac_plan(const std::vector<MacStream> &ss, const u64 *q, int nlimbs, size_t n, int kara_switch)
{
    MacPlan p;
    p.nlimbs = nlimbs; p.n = n;
    // streams are generated bundle-major; match each stream with later ones of equal key
    std::vector<size_t> order(ss.size());
    for (size_t i = 0; i < ss.size(); i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
        if (ss[a].pw != ss[b].pw) return ss[a].pw < ss[b].pw;
        if (ss[a].limb0 != ss[b].limb0) return ss[a].limb0 < ss[b].limb0;
        if (ss[a].nl != ss[b].nl) return ss[a].nl < ss[b].nl;
        return ss[a].cnt < ss[b].cnt;
    });
    for (size_t x = 0; x < order.size();) {
        const MacStream &f = ss[order[x]];
        MacJob j{};
        j.pw = f.pw; j.cnt = f.cnt; j.pt_stride = f.pt_stride; j.pw_stride = f.pw_stride; j.pw_poly_stride = f.pw_poly_stride;
        j.out_poly_stride = f.out_poly_stride; j.limb0 = f.limb0; j.nl = f.nl; j.packed = f.packed;
        u32 g = 0;
        while (x < order.size() && g < (u32)MAC_G) {
            const MacStream &s = ss[order[x]];
            if (s.pw != f.pw || s.cnt != f.cnt || s.packed != f.packed || s.pt_stride != f.pt_stride || s.pw_stride != f.pw_stride ||
                s.pw_poly_stride != f.pw_poly_stride || s.out_poly_stride != f.out_poly_stride || s.limb0 != f.limb0 || s.nl != f.nl) break;
            j.pt[g] = s.pt; j.out[g] = s.out; g++; x++;
        }
        j.ng = g;
        for (u32 r = g; r < (u32)MAC_G; r++) { j.pt[r] = j.pt[0]; j.out[r] = j.out[0]; }
        p.jobs.push_back(j);
    }
    uint64_t terms = 0, chains = 0;
    for (auto &j : p.jobs) {
        uint64_t w = 0;
        for (u32 l = j.limb0; l < j.limb0 + j.nl; l++) w += j.packed ? packed_row_bits(q[l]) : 64;
        p.units += (uint64_t)j.cnt * j.ng * w;
        terms += (uint64_t)j.cnt * j.ng * j.nl; chains += (uint64_t)j.ng * j.nl;
    }
    p.mean_cnt = chains ? (uint32_t)(terms / chains) : 0;
    p.packed = !p.jobs.empty() && p.jobs[0].packed != 0;
    p.kara = !(kara_switch == 0 || (kara_switch < 0 && p.mean_cnt < 96));
    for (int j = 0; j < nlimbs && p.kara; j++) p.kara = mac_kara_usable(q[j]);
    p.grid = mac_grid(n, p.jobs.size());
    return p;
}

} // namespace apsu_he
