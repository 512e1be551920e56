// CPU emulation, the multiply-accumulate family (mac_core.h: the functions the kernels run, stepped over every lane of a launch's grid;
// mac_plan.h).  Held to big-integer sums by tests/test_mac_core_cpu.py.
#include <cstring>
#include <stdexcept>
#include <vector>

#include "emu_common.h"
#include "mac_core.h"
#include "mac_plan.h"

using namespace apsu_he;

// A level of nl limbs whose k_mac constants are GIVEN, so that a test can pass wrong ones: per limb the modulus, the split width, the
// chunk of either form and the row width in bits (64: dense); n lays the packed rows out.
static DevLevel mac_level(int nl, const uint64_t *q, const uint32_t *shift, const uint32_t *chunk, const uint32_t *chunk_k, const uint32_t *bits, size_t n)
{
    if (nl < 1 || nl > DMAXL) throw std::invalid_argument("limbs");
    DevLevel d;
    std::memset(&d, 0, sizeof(d));
    d.L = nl;
    for (int j = 0; j < nl; j++) {
        d.q[j] = make_mod(q[j]);
        d.mac_shift[j] = shift[j]; d.mac_chunk[j] = chunk[j]; d.mac_chunk_k[j] = chunk_k[j];
        d.mac_bits[j] = bits[j];
        d.mac_row_off[j] = j ? d.mac_row_off[j - 1] + (u32)(n * bits[j - 1] / 8) : 0;
        d.mac_mask_hi[j] = mac_mask_hi_of(bits[j], (int)shift[j]);
    }
    return d;
}
template <bool KARA, bool PACKED> static void emu_mac_grid(const DevLevel &lv, const MacJob *jobs, size_t n, int njobs, int limb_slow)
{
    const unsigned gx = mac_grid(n, (size_t)njobs).gx, gl = (unsigned)lv.L, gj = (unsigned)njobs;
    const unsigned gy = limb_slow ? gj : gl, gz = limb_slow ? gl : gj;            // launch_mac's two grids
    for (unsigned bz = 0; bz < gz; bz++)
        for (unsigned by = 0; by < gy; by++)
            for (unsigned bx = 0; bx < gx; bx++)
                for (unsigned tx = 0; tx < (unsigned)EW_T; tx++) k_mac<KARA, PACKED>(&lv, jobs, n, limb_slow, bx, by, bz, tx);
}
extern "C" {

// k_mac over njobs jobs (MacJob as the device reads it, emu_mac_job_bytes) in either form and either grid order
int emu_mac(int nl, const uint64_t *q, const uint32_t *shift, const uint32_t *chunk, const uint32_t *chunk_k, const uint32_t *bits, uint64_t n,
            const void *jobs, int njobs, int kara, int packed, int limb_slow)
{
    return guarded([&]() -> int {
        const DevLevel lv = mac_level(nl, q, shift, chunk, chunk_k, bits, n);
        const MacJob *mj = static_cast<const MacJob *>(jobs);
        if (packed) { if (kara) emu_mac_grid<true, true>(lv, mj, n, njobs, limb_slow); else emu_mac_grid<false, true>(lv, mj, n, njobs, limb_slow); }
        else if (kara) emu_mac_grid<true, false>(lv, mj, n, njobs, limb_slow);
        else emu_mac_grid<false, false>(lv, mj, n, njobs, limb_slow);
        return 0;
    });
}
int emu_mac_job_bytes() { return (int)sizeof(MacJob); }
// k_term_product over njobs TermJobs {pt, pw, out} on limb `limb`
int emu_term_product(int nl, const uint64_t *q, const uint32_t *shift, const uint32_t *chunk, const uint32_t *chunk_k, const uint32_t *bits, uint64_t n,
                     const void *jobs, uint64_t njobs, int limb, uint32_t pw_poly_stride, uint32_t out_poly_stride, int packed)
{
    return guarded([&]() -> int {
        const DevLevel lv = mac_level(nl, q, shift, chunk, chunk_k, bits, n);
        const TermJob *tj = static_cast<const TermJob *>(jobs);
        const size_t lanes = (n / 2 + EW_T - 1) / EW_T * EW_T;                   // launch_term_product's grid: x, and the jobs over y and z --
        const size_t gy = njobs < 32768 ? njobs : 32768, gz = gy ? (njobs + gy - 1) / gy : 0;   // the last z slab is stepped whole, beyond njobs
        for (size_t u = 0; u < gy * gz; u++)
            for (size_t t = 0; t < lanes; t++) {
                if (packed) term_product_lane<true>(&lv, tj, njobs, n, limb, pw_poly_stride, out_poly_stride, t * 2, u);
                else term_product_lane<false>(&lv, tj, njobs, n, limb, pw_poly_stride, out_poly_stride, t * 2, u);
            }
        return 0;
    });
}
// k_pack_rows / k_unpack_rows over `slots` slots of L limbs (the level's first L row widths), behind the host check that stands in front
// of every launch of them (pack_rows_grid_check, mac_plan.h: -1 with its refusal, before an array is touched)
int emu_pack_rows(int L, const uint32_t *bits, uint64_t n, const uint64_t *dense, void *packed, uint64_t slot_bytes, uint64_t slots, int unpack, uint64_t *dense_out)
{
    return guarded([&]() -> int {
        pack_rows_grid_check(slots, L);
        std::vector<uint64_t> q(L, 3); std::vector<uint32_t> z(L, 1);
        const DevLevel lv = mac_level(L, q.data(), z.data(), z.data(), z.data(), bits, n);
        const size_t lanes = ((unpack ? n : n * 2) + EW_T - 1) / EW_T * EW_T;     // launch_pack_rows / launch_unpack_rows
        for (unsigned by = 0; by < (unsigned)(slots * L); by++)                  // the kernels' blockIdx.y
            for (size_t t = 0; t < lanes; t++) {
                if (unpack) unpack_rows_lane(&lv, L, static_cast<const char *>(packed), slot_bytes, dense_out, n, t, by / L, (int)(by % L));
                else pack_rows_lane(&lv, L, dense, static_cast<char *>(packed), slot_bytes, n, t, by / L, (int)(by % L));
            }
        return 0;
    });
}
uint32_t emu_packed_row_bits(uint64_t q) { return packed_row_bits(q); }
uint64_t emu_packed_coeff(const uint32_t *row, uint64_t c, uint32_t w) { return packed_coeff(row, c, w); }
// coefficients k, k + 1 (k even) of a row of kb-bit coefficients through the 16-byte window a lane of k_mac / k_term_product loads
void emu_packed_pair(const void *row, uint64_t k, uint32_t kb, uint64_t *out)
{
    u32 psh;
    const u32x4a4 w = ldg16_a4_nt(packed_window(row, 0, k, kb, psh));
    packed_pair((u64)w[0] | ((u64)w[1] << 32), (u64)w[2] | ((u64)w[3] << 32), psh, kb, out[0], out[1]);
}
// the rules of the modulus: out = { shift, chunk, chunk of the three-product form, that form usable }
void emu_mac_rules(uint64_t q, uint32_t *out)
{
    out[0] = (uint32_t)mac_shift_of(q); out[1] = mac_chunk_of(q); out[2] = mac_chunk_k_of(q); out[3] = mac_kara_usable(q) ? 1 : 0;
}
// mac_plan: streams [ns][11] = { pt, pw, out, cnt, pt_stride, pw_stride, pw_poly_stride, out_poly_stride, limb0, nl, packed };
// jobs (may be NULL): room for `cap` MacJobs; info = { jobs, units, mean chain length, three-product, packed, gx, limb_slow }
int emu_mac_plan(const uint64_t *streams, uint64_t ns, const uint64_t *q, int nlimbs, uint64_t n, int kara_switch, void *jobs, uint64_t cap, uint64_t *info)
{
    return guarded([&]() -> int {
        std::vector<MacStream> ss(ns);
        for (size_t i = 0; i < ns; i++) {
            const uint64_t *s = streams + i * 11;
            ss[i] = MacStream{ reinterpret_cast<const u64 *>(s[0]), reinterpret_cast<const u64 *>(s[1]), reinterpret_cast<u64 *>(s[2]), (u32)s[3], (u32)s[4],
                               (u32)s[5], (u32)s[6], (u32)s[7], (u32)s[8], (u32)s[9], (u32)s[10] };
        }
        const MacPlan p = mac_plan(ss, q, nlimbs, n, kara_switch);
        if (jobs) { if (p.jobs.size() > cap) throw std::invalid_argument("job buffer too small"); std::memcpy(jobs, p.jobs.data(), p.jobs.size() * sizeof(MacJob)); }
        const uint64_t v[7] = { p.jobs.size(), p.units, p.mean_cnt, p.kara, p.packed, p.grid.gx, (uint64_t)p.grid.limb_slow };
        for (int i = 0; i < 7; i++) info[i] = v[i];
        return 0;
    });
}

} // extern "C"
