// CPU emulation, reading the bins back and splitting them (kernels_roots.hip's headers: bin_roots.h, bin_split.h).  The coset transforms
// run through the workgroup driver (ntt_driver.h) with the source SrcCoset, as k_bin_roots runs them through ntt_body.
#include <algorithm>

#include "emu_common.h"
#include "ntt_driver.h"
#include "bin_roots.h"
#include "bin_split.h"

using namespace apsu_he;

extern "C" {

// ---- reading the bins back (bin_roots.h)
uint64_t emu_field_generator(uint64_t t)
{
    try { return field_generator(t); } catch (const std::exception &e) { g_err = e.what(); return 0; }
}

// (t - 1) / n, or -1 with emu_last_error for a modulus the walk cannot serve
int64_t emu_roots_coset_count(uint64_t t, uint64_t n)
{
    return guarded([&]() -> int64_t { return (int64_t)roots_coset_count(t, n); });
}

int emu_ntt_limb_c(int logn, int inverse, uint64_t q, uint64_t *data, int threads, int coeffs);
// the point table: the forward transform mod t of the polynomial X, through the library transform's emulation
int emu_roots_points(int logn, uint64_t t, uint64_t *pts)
{
    const size_t n = (size_t)1 << logn;
    std::fill(pts, pts + n, 0);
    pts[1] = 1;
    return emu_ntt_limb_c(logn, 0, t, pts, (int)std::max<size_t>(64, n / 16), 16);
}

// the coset walk alone: out[j * n + k] = c_j pts[k], the evaluation point of output position k of coset j, j < (t - 1) / n
int emu_roots_walk(int logn, uint64_t t, uint64_t *out)
{
    return guarded([&]() -> int {
        const size_t n = (size_t)1 << logn;
        const u32 cosets = roots_coset_count(t, n);
        const u64 g = field_generator(t), r1 = (u64)((((unsigned __int128)1) << 64) / t);
        std::vector<u64> pts(n);
        if (emu_roots_points(logn, t, pts.data())) return -1;
        u64 c = roots_coset_before(g, 0, t, r1);
        for (u32 j = 0; j < cosets; j++) {
            c = roots_mul(c, g, t, r1);
            for (size_t k = 0; k < n; k++) out[(size_t)j * n + k] = roots_value(c, pts[k], t, r1);
        }
        return 0;
    });
}

// k_bin_roots and k_roots_mult on ONE bin, as the workgroups and the wave run them: col[rows] are the bin's coefficients mod t (the
// count is the index of the highest non-zero one), `blocks` the number of coset blocks the bin's cosets are split into (each block a
// work item of its own, with its own scaled load).  values / mult [cap]: the distinct roots in the order found and their
// multiplicities; returns how many were found, -1 (emu_last_error) on a refusal.  cap >= count.
int64_t emu_bin_roots(int logn, uint64_t t, const uint64_t *col_in, uint32_t rows, uint32_t blocks, uint64_t *values, uint32_t *mult, uint32_t cap)
{
    return guarded([&]() -> int64_t {
        const size_t n = (size_t)1 << logn;
        const u32 cosets = roots_coset_count(t, n);
        int top = (int)rows - 1;
        while (top >= 0 && col_in[top] == 0) top--;
        if (top < 0) throw std::invalid_argument("the zero polynomial is not a bin");
        const u32 cnt = (u32)top;
        if (cnt >= n) throw std::invalid_argument("degree does not fit one transform");
        if (cap < cnt) throw std::invalid_argument("cap below the count");
        if (!blocks || blocks > cosets) throw std::invalid_argument("blocks out of range");
        const int T = (int)std::max<size_t>(64, n / 16);
        const EmuTables et(logn, t);
        const NttTable &tab = et.tab;
        const u64 q = tab.q, r1 = tab.r1, g = field_generator(t);
        const std::vector<u32> step = roots_step_table(g, t, n);
        std::vector<u64> pts(n), col(col_in, col_in + rows);
        if (emu_roots_points(logn, t, pts.data())) return -1;
        RootsGrid grid;
        grid.per_block = (cosets + blocks - 1) / blocks;
        grid.blocks = (cosets + grid.per_block - 1) / grid.per_block;
        u32 found = 0;
        if (cnt >= 1) {                                              // an occupied bin: the work items of k_bin_roots
            std::vector<u32> v(n);
            std::vector<u64> row(n);
            for (u32 blk = 0; blk < grid.blocks; blk++) {
                const u32 j0 = blk * grid.per_block, j1 = std::min(cosets, j0 + grid.per_block);
                u64 c = roots_coset_before(g, j0, q, r1);
                for (int tid = 0; tid < T; tid++)
                    for (int e = tid; e < (int)n; e += T) v[e] = (u32)e <= cnt ? (u32)roots_scaled_load(col[e], c, (u32)e, q, r1) : 0;
                if (blk == 0 && roots_is_zero(col[0])) roots_append(&found, values, cnt, 0);
                for (u32 j = j0; j < j1; j++) {
                    c = roots_mul(c, g, q, r1);
                    const SrcCoset ops{ v.data(), step.data() };
                    if (logn == 11 || logn == 14) throw std::invalid_argument("unsupported logn");     // (ring sizes this call has never served)
                    // the forward transform whose load steps v to the next coset, as k_bin_roots instantiates ntt_body
                    emu_with_shape(logn, 16, [&](auto ln, auto) {
                        emu_ntt_body<decltype(ln)::value, false, NTT_NARROW, 0, false, SrcCoset>(row.data(), tab, T, nullptr, ops);
                    });
                    for (int tid = 0; tid < T; tid++)
                        for (int e = tid; e < (int)n; e += T)
                            if (roots_is_zero(row[e])) roots_append(&found, values, cnt, roots_value(c, pts[e], q, r1));
                }
            }
        }
        // k_roots_mult: the wave of this bin
        const u32 nf = std::min(found, cnt);
        if (nf < cnt) {
            u32 top_now = cnt;
            for (u32 base = 0; base < nf; base += ROOTS_LANES) {
                u64 r[ROOTS_LANES], b1s[ROOTS_LANES];
                bool live[ROOTS_LANES];
                for (u32 lane = 0; lane < ROOTS_LANES; lane++) {
                    live[lane] = base + lane < nf;
                    r[lane] = live[lane] ? values[base + lane] : 0;
                    u64 b0 = 0, b1 = 0;
                    for (int d = (int)cnt; d >= 0; d--) roots_deriv_step(b0, b1, r[lane], col[d], q, r1);
                    b1s[lane] = b1;
                    if (live[lane] && b1 != 0) mult[base + lane] = 1;
                }
                for (u32 l = 0; l < ROOTS_LANES; l++) {               // the ballot's bits, lowest first; lane 0 works
                    if (!(live[l] && b1s[l] == 0)) continue;
                    const u64 a = r[l];
                    u32 m = 0;
                    for (;;) {
                        u64 rem = 0;
                        for (int k = (int)top_now; k >= 0; k--) rem = roots_div_step(col[k], a, rem, q, r1);
                        if (rem != 0 || top_now == 0) break;
                        u64 sv = 0;
                        for (int k = (int)top_now; k >= 0; k--) {
                            const u64 pk = col[k];
                            col[k] = sv;
                            sv = roots_div_step(pk, a, sv, q, r1);
                        }
                        top_now--;
                        m++;
                    }
                    mult[base + l] = m;
                }
            }
        } else std::fill(mult, mult + nf, 1u);
        return (int64_t)found;
    });
}

// the host end of the call (roots_expand): out[count] = the sorted multiset, or -1 with the refusal in emu_last_error
int emu_roots_expand(uint32_t slot, uint32_t count, const uint64_t *values, const uint32_t *mult, uint32_t found, uint64_t *out)
{
    return guarded([&]() -> int {
        std::vector<u64> v;
        roots_expand(slot, count, values, mult, found, v);
        std::copy(v.begin(), v.end(), out);
        return 0;
    });
}

// ---- splitting and moving (bin_split.h, db_rebase.h)
uint32_t emu_split_cut(uint32_t c, uint32_t k, uint32_t p) { return split_cut(c, k, p); }
uint32_t emu_split_part_of(uint32_t c, uint32_t k, uint32_t pos) { return split_part_of(c, k, pos); }
uint32_t emu_split_capacity(uint32_t hstride) { return split_capacity(hstride); }
// the number of parts, or -1 with emu_last_error
int64_t emu_split_parts(uint32_t max_count, uint32_t limit)
{
    return guarded([&]() -> int64_t { return (int64_t)split_parts(max_count, limit); });
}

// k_roots_split as its workgroups run it, one after the other: the launcher's arguments on host arrays (launch_roots.h: launch_roots_split,
// the zeroing of counts_out included).  *failure: SPLIT_NO_FAILURE beforehand, as on the device.  Returns 0, -1 for what the launcher refuses.
int emu_roots_split(const uint64_t *hits, const uint32_t *found, const uint32_t *mult, uint32_t hstride, const uint32_t *occ, const uint32_t *counts,
                    uint32_t n_occ, uint32_t k, uint64_t *out, const uint64_t *part_off, const uint32_t *part_stride, uint32_t *counts_out, uint32_t cstride,
                    uint64_t *failure)
{
    return guarded([&]() -> int {
        split_emulate(hits, found, mult, hstride, occ, counts, n_occ, k, out, part_off, part_stride, counts_out, cstride, failure);
        return 0;
    });
}

} // extern "C"
