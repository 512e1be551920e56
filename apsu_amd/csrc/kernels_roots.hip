// Reading the bins of a resident BinBundle back from its polynomials (Engine::bundle_bins), a translation unit of its own: the
// transforms' object (kernels_ntt.hip) is built exactly as before.  Rules and lane arithmetic: bin_roots.h, which the CPU tier runs as well.
// Input of every kernel here: poly[d][slot], the slot values mod t that Engine::decode_bundle produces; bin s is the column s, read
// top down to its count.
// Also here, on the same input: the plaintext answer of a BinBundle and the self-test's comparison (k_bins_eval, k_eval_compare; bin_eval.h).
#include "launch_roots.h"
#include "kernel_launch.h"
#include "ntt_wg.h"
#include "bin_rows.h"
#include "bin_eval.h"
#include "bin_split.h"

namespace apsu_he {

// ---- the persistent kernel.  A work item is (occupied bin, block of consecutive cosets); a workgroup takes work items blockIdx.x,
// blockIdx.x + gridDim.x, ...  It reads the bin's column ONCE, keeps the scaled coefficients v_i (32-bit words) in its own row of
// `vrows` (32 KiB at n = 8192, read and written by this workgroup alone: L2-resident.  In LDS next to the transform's image they cost the
// second workgroup per CU at n = 8192 -- 104 KiB -- and the search took 1.13 x (16M-4096) to 1.27 x (256M-4096) as long, profiles/r15_bundle_bins.txt), and for each coset of its block steps v to that coset while the transform loads it (SrcCoset), runs the workgroup
// transform of ntt_wg.h in the throughput form (16 coefficients per lane), and tests the n outputs for zero.  The transform's closing
// reduction leaves canonical residues in the workgroup's own row of `rows` (n words, written and read back by the same workgroup: it
// stays in the L2); a zero at position k is the root c_j pts[k], appended to the bin's list through the bin's counter.  Nothing but
// the hits goes to memory.  The root 0 lies in no coset: a_0 = 0 is tested by the bin's first block.
// rows: [gridDim.x][n] u64, vrows: [gridDim.x][n] u32; hits: [n_occupied][hstride], found: [n_occupied] (zeroed); hstride >= every count.
template <int LOGN, int T, int MINW>
__global__ __launch_bounds__(T, MINW) void k_bin_roots(const u64 *__restrict__ poly, const u32 *__restrict__ occ, const u32 *__restrict__ counts, u32 n_work,
                                                    RootsGrid grid, u32 cosets, const NttTable *__restrict__ tabs, const int *__restrict__ modmap,
                                                    const u32 *__restrict__ step, const u64 *__restrict__ pts, u64 g, u64 *__restrict__ rows,
                                                    u32 *__restrict__ vrows, u64 *__restrict__ hits, u32 *__restrict__ found, u32 hstride)
{
    constexpr int N = 1 << LOGN;
    __shared__ __attribute__((aligned(16))) u64 lds[lds_slots(N)];
    const int tid = threadIdx.x;
    const NttTable tab = tabs[modmap[0] & NTT_MAP_MASK];
    const u64 q = tab.q, r1 = tab.r1;
    u64 *p = rows + (size_t)blockIdx.x * N;
    u32 *v = vrows + (size_t)blockIdx.x * N;
    for (u32 w = blockIdx.x; w < n_work; w += gridDim.x) {           // workgroup-uniform
        const u32 rank = w / grid.blocks, blk = w - rank * grid.blocks;
        const u32 s = occ[rank], cnt = counts[s];
        const u32 j0 = blk * grid.per_block, j1 = min(cosets, j0 + grid.per_block);
        u64 c = roots_coset_before(g, j0, q, r1);
        u64 *list = hits + (size_t)rank * hstride;
        __syncthreads();                                             // the transform before has read v
        for (int e = tid; e < N; e += T) v[e] = (u32)e <= cnt ? (u32)roots_scaled_load(poly[(size_t)e * N + s], c, (u32)e, q, r1) : 0;
        if (blk == 0 && tid == 0 && roots_is_zero(poly[s])) roots_append(found + rank, list, cnt, 0);
        __syncthreads();
        for (u32 j = j0; j < j1; j++) {
            c = roots_mul(c, g, q, r1);                              // c_j
            ntt_body<LOGN, false, NTT_NARROW, T, 0, false, SrcCoset>(lds, p, tab, tid, nullptr, SrcCoset{ v, step });
            __syncthreads();                                         // the row is complete
            for (int e = tid; e < N; e += T)
                if (roots_is_zero(p[e])) roots_append(found + rank, list, cnt, roots_value(c, pts[e], q, r1));
            __syncthreads();                                         // before the next transform writes the image and the row
        }
    }
}

// ---- the plain composition (rings without an LDS-resident transform form here, and the form the persistent kernel is tested
// against): per coset one transposed-and-scaled gather into [bin][n] limb rows, the library's forward transform mod t, one scan.
__global__ __launch_bounds__(EW_T) void k_roots_gather(const u64 *__restrict__ poly, size_t n, const u32 *__restrict__ occ, const u32 *__restrict__ counts,
                                                       u64 c, Mod t, u64 *__restrict__ rows)
{
    const size_t i = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const u32 s = occ[blockIdx.y], cnt = counts[s];
    rows[(size_t)blockIdx.y * n + i] = i <= cnt ? roots_scaled_load(poly[i * n + s], c, (u32)i, t.q, t.r1) : 0;
}

__global__ __launch_bounds__(EW_T) void k_roots_scan(const u64 *__restrict__ rows, size_t n, const u64 *__restrict__ pts, u64 c, Mod t, int first,
                                                     const u64 *__restrict__ poly, const u32 *__restrict__ occ, const u32 *__restrict__ counts,
                                                     u64 *__restrict__ hits, u32 *__restrict__ found, u32 hstride)
{
    const size_t i = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const u32 rank = blockIdx.y, s = occ[rank], cnt = counts[s];
    u64 *list = hits + (size_t)rank * hstride;
    if (first && i == 0 && roots_is_zero(poly[s])) roots_append(found + rank, list, cnt, 0);
    if (roots_is_zero(rows[(size_t)rank * n + i])) roots_append(found + rank, list, cnt, roots_value(c, pts[i], t.q, t.r1));
}

// ---- multiplicities: one WAVE per occupied bin, which leaves at once unless the bin has fewer distinct roots than items.  Lane =
// found root, 64 at a time: P(r) and P'(r) by one Horner walk down the column (every lane reads the same coefficient: one broadcast
// load per row).  A root with P'(r) != 0 is simple.  For the others lane 0 divides the column by (x - r) in place as long as the
// remainder is 0 (poly is the call's own decoded copy); dividing out one root's factors leaves every other root's multiplicity alone.
// mult: [n_occupied][hstride], written for every found root of a bin with a deficit (the host takes 1 elsewhere).
__global__ __launch_bounds__(256) void k_roots_mult(u64 *__restrict__ poly, size_t n, const u32 *__restrict__ occ, const u32 *__restrict__ counts, u32 n_occ,
                                                    Mod t, const u64 *__restrict__ hits, const u32 *__restrict__ found, u32 *__restrict__ mult, u32 hstride)
{
    const u32 lane = threadIdx.x & 63;
    const u32 rank = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (rank >= n_occ) return;
    const u32 s = occ[rank], cnt = counts[s], nf = min(found[rank], cnt);
    if (nf >= cnt) return;                                           // as many distinct roots as items: all simple
    u64 *col = poly + s;
    const u64 q = t.q, r1 = t.r1;
    u32 top = cnt;                                                   // degree of what the column holds now (lane 0's)
    for (u32 base = 0; base < nf; base += ROOTS_LANES) {
        const bool live = base + lane < nf;
        const u64 r = live ? hits[(size_t)rank * hstride + base + lane] : 0;
        u64 b0 = 0, b1 = 0;
        for (int d = (int)cnt; d >= 0; d--) roots_deriv_step(b0, b1, r, col[(size_t)d * n], q, r1);
        if (live && b1 != 0) mult[(size_t)rank * hstride + base + lane] = 1;
        unsigned long long multiple = __ballot(live && b1 == 0);
        while (multiple) {                                           // wave-uniform
            const int l = __ffsll(multiple) - 1;
            multiple &= multiple - 1;
            const u64 a = __shfl((unsigned long long)r, l, 64);
            if (lane == 0) {
                u32 m = 0;
                for (;;) {
                    u64 rem = 0;
                    for (int k = (int)top; k >= 0; k--) rem = roots_div_step(col[(size_t)k * n], a, rem, q, r1);
                    if (rem != 0 || top == 0) break;
                    u64 sv = 0;
                    for (int k = (int)top; k >= 0; k--) {
                        const u64 pk = col[(size_t)k * n];
                        col[(size_t)k * n] = sv;
                        sv = roots_div_step(pk, a, sv, q, r1);
                    }
                    top--;
                    m++;
                }
                mult[(size_t)rank * hstride + base + l] = m;
            }
            __threadfence_block();                                   // the other lanes' next walk reads what lane 0 wrote
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// ---- the bins' polynomials as ragged rows (Engine::export_saved; bin_rows.h): out[off[s] + d] = poly[d][s], d <= counts[s], for the
// first `bins` slots.  One workgroup per tile of 64 slots x 64 degrees: row segments in (lane = slot), row segments out (lane =
// degree), through a padded LDS tile.  tops: per tile of slots the largest count, -1 for none.  Nothing at or behind off[bins] is written.
__global__ __launch_bounds__(ROWS_TILE * ROWS_WAVES) void k_bins_rows(const u64 *__restrict__ poly, size_t n, u32 rows, const u32 *__restrict__ counts,
                                                                      const u64 *__restrict__ off, const int *__restrict__ tops, u32 bins,
                                                                      u64 *__restrict__ out)
{
    __shared__ u64 tile[ROWS_LDS_WORDS];
    const int lane = threadIdx.x & (ROWS_TILE - 1), wave = threadIdx.x / ROWS_TILE;
    const size_t s0 = (size_t)blockIdx.x * ROWS_TILE;
    const u32 d0 = blockIdx.y * ROWS_TILE;
    const int top = tops[blockIdx.x];
    if ((int)d0 > top) return;                                       // workgroup-uniform: no bin of this tile reaches these degrees
    for (int dl = wave; dl < ROWS_TILE; dl += ROWS_WAVES)
        if (rows_load_live(d0 + dl, s0 + lane, rows, n, top)) tile[rows_lds_at(dl, lane)] = poly[(size_t)(d0 + dl) * n + s0 + lane];
    __syncthreads();
    for (int sl = wave; sl < ROWS_TILE; sl += ROWS_WAVES) {
        const size_t s = s0 + sl;
        if (s >= bins) break;                                        // wave-uniform
        if (rows_store_live(d0 + lane, s, counts[s], bins)) out[off[s] + d0 + lane] = tile[rows_lds_at(lane, sl)];
    }
}

// ---- what the BinBundle answers in plaintext (Engine::bundles_eval_plain, Engine::self_test; bin_eval.h): out[s] = P_s(x[s]) + mask[s] mod t
// for every slot, P_s the column s of poly[rows][n].  Lane = slot: one WAVE per tile of 64 consecutive slots, rows d = top .. 0 with one
// contiguous 512-byte segment per d, EVAL_ROWS of them loaded before their Horner steps; top = the largest count of the tile, the
// maximum over the wave of k_bin_counts' output.  One point per slot, so a stored coefficient is read exactly once.  mask and is_bin
// may be null.  A slot or mask value that is not below t raises *bad (a plain store of 1: whoever finds one writes the same word).
// No LDS, no atomics; every word of out (and of is_bin) is written by exactly one lane.
template <bool NARROW>
__global__ __launch_bounds__(EVAL_LANES) void k_bins_eval(const u64 *__restrict__ poly, size_t n, u32 rows, const u32 *__restrict__ counts,
                                                          const u64 *__restrict__ x, const u64 *__restrict__ mask, Mod t, u64 *__restrict__ out,
                                                          unsigned char *__restrict__ is_bin, u32 *__restrict__ bad)
{
    const size_t slot = (size_t)blockIdx.x * EVAL_LANES + threadIdx.x;
    const bool live = slot < n;                                   // (n < 64 only)
    const u32 cnt = live ? counts[slot] : LOOKUP_NONE;
    int top = eval_count_top(cnt);
#pragma unroll
    for (int m = EVAL_LANES / 2; m; m >>= 1) top = max(top, __shfl_xor(top, m, EVAL_LANES));
    const u64 *col = poly + (live ? slot : 0);
    const u64 xs = live ? x[slot] : 0;
    const u64 acc = eval_walk<NARROW>(col, n, eval_walk_top(top, rows), xs, t);      // the top is wave-uniform
    if (!live) return;
    const u64 ms = mask ? mask[slot] : 0;
    if (xs >= t.q || ms >= t.q) *bad = 1;
    out[slot] = eval_finish(acc, ms, t);
    if (is_bin) is_bin[slot] = eval_is_bin(cnt) ? 1 : 0;
}

// the self-test's comparison of what was decrypted with what the polynomials say: got, want [count][n].  One lane per slot (grid.y = the
// BinBundle's position); status[0] += the workgroup's mismatches (one atomic per workgroup that has any), status[1] = min of
// (position << 32 | slot) over the mismatches (EVAL_NO_MISMATCH beforehand).
__global__ __launch_bounds__(EW_T) void k_eval_compare(const u64 *__restrict__ got, const u64 *__restrict__ want, size_t n, unsigned long long *__restrict__ status)
{
    const size_t i = (size_t)blockIdx.x * EW_T + threadIdx.x;
    const bool bad = i < n && got[(size_t)blockIdx.y * n + i] != want[(size_t)blockIdx.y * n + i];
    if (bad) atomicMin(status + 1, (unsigned long long)eval_mismatch_key(blockIdx.y, (u32)i));
    const int total = __syncthreads_count(bad);
    if (total && threadIdx.x == 0) atomicAdd(status, (unsigned long long)total);
}

// ---- the bins of a BinBundle cut into k parts on the device (Engine::split_bundle; bin_split.h): behind k_roots_mult, one WORKGROUP per
// occupied bin.  The bin's distinct roots and multiplicities become 64-bit keys in LDS (CAP of them, the rest sentinels), a bitonic
// network sorts them, every work item then takes CAP / T consecutive keys into registers and the key array's first words serve the
// workgroup scan of the multiplicities.  A bin whose multiplicities do not add up to its count reports split_failure by atomicMin and
// writes nothing; every other bin writes each part's items to the part's row of the bin and each part's count.  Words behind a part's
// count, and rows and counts of slots that are not in occ, are not written.  LDS: CAP keys, dynamic (64 KiB in the largest instance).
template <int CAP, int T>
__global__ __launch_bounds__(T) void k_roots_split(const u64 *__restrict__ hits, const u32 *__restrict__ found, const u32 *__restrict__ mult, u32 hstride,
                                                   const u32 *__restrict__ occ, const u32 *__restrict__ counts, u32 k, u64 *__restrict__ out,
                                                   const u64 *__restrict__ part_off, const u32 *__restrict__ part_stride, u32 *__restrict__ counts_out,
                                                   u32 cstride, unsigned long long *__restrict__ failure)
{
    constexpr int PER = CAP / T, WAVES = T / 64;
    static_assert(PER * T == CAP && WAVES * 64 == T && CAP >= 2 * WAVES, "k_roots_split: the instance's shape");
    __shared__ __attribute__((aligned(16))) u64 key[CAP];
    const u32 tid = threadIdx.x, rank = blockIdx.x;
    const u32 slot = occ[rank], cnt = counts[slot], nf = found[rank];
    const u64 *list = hits + (size_t)rank * hstride;
    const u32 *ml = mult + (size_t)rank * hstride;
    for (u32 i = tid; i < (u32)CAP; i += T) key[i] = i < hstride ? split_load(list, ml, i, nf, cnt) : SPLIT_SENTINEL;
    __syncthreads();
    for (u32 size = 2; size <= (u32)CAP; size <<= 1)
        for (u32 j = size >> 1; j; j >>= 1) {
            for (u32 i = tid; i < (u32)CAP / 2; i += T) {
                u32 lo, hi;
                split_pair(i, j, lo, hi);
                u64 a = key[lo], b = key[hi];
                split_exchange(a, b, split_ascending(lo, size));
                key[lo] = a;
                key[hi] = b;
            }
            __syncthreads();
        }
    u64 mine[PER];
    u32 sum = 0;
#pragma unroll
    for (int e = 0; e < PER; e++) {
        mine[e] = key[tid * PER + e];
        sum = split_combine(sum, split_key_mult(mine[e]));
    }
    __syncthreads();                                                 // the keys are in registers: the array's first words become the scan's
    u32 incl = sum;                                                  // inclusive scan over the wave, then over the waves' totals
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 up = __shfl_up(incl, d, 64);
        if ((int)(tid & 63) >= d) incl = split_combine(incl, up);
    }
    u32 *wave_total = reinterpret_cast<u32 *>(key);
    if ((tid & 63) == 63) wave_total[tid >> 6] = incl;
    __syncthreads();
    u32 before = 0, total = 0;
    for (int w = 0; w < WAVES; w++) {
        const u32 x = wave_total[w];
        if (w < (int)(tid >> 6)) before = split_combine(before, x);
        total = split_combine(total, x);
    }
    if (!split_bin_ok(nf, cnt, total)) {                             // workgroup-uniform
        if (tid == 0) atomicMin(failure, (unsigned long long)split_failure(slot, nf, cnt, total));
        return;
    }
    u32 pos = split_combine(before, incl - sum);
#pragma unroll
    for (int e = 0; e < PER; e++) {
        const u32 m = split_key_mult(mine[e]);
        split_write(out, part_off, part_stride, slot, cnt, k, pos, m, split_key_value(mine[e]));
        pos = split_combine(pos, m);
    }
    for (u32 p = tid; p < k; p += T) counts_out[(size_t)p * cstride + slot] = split_cut(cnt, k, p + 1) - split_cut(cnt, k, p);
}

// ---- launches
// workgroups a CU holds: two at n = 8192 (72 KiB of LDS each, 126 VGPRs: 4 waves per SIMD), two at 4096 (170 VGPRs: 2 waves per SIMD; a
// budget of 168 or 128 registers spills there); resource report: profiles/r15_bundle_bins.txt
static int roots_wgs_per_cu(int logn) { return logn >= 13 ? 2 : logn == 12 ? 2 : 8; }

bool bin_roots_has_kernel(int logn) { return logn == 13 || logn == 12 || logn == 6; }

u32 bin_roots_wg_slots(int logn)
{
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 1;
    return (u32)cus * (u32)roots_wgs_per_cu(logn);
}

void launch_bin_roots(int logn, const u64 *poly, const u32 *occ, const u32 *counts, u32 n_occ, RootsGrid grid, u32 cosets, u32 wgs, const NttTable *tabs,
                      const int *modmap, const u32 *step, const u64 *pts, u64 g, u64 *rows, u32 *vrows, u64 *hits, u32 *found, u32 hstride, hipStream_t st)
{
    const u32 n_work = n_occ * grid.blocks;
    if (!n_work) return;
#define BR_CASE(LN, T, W) case LN: hipLaunchKernelGGL((k_bin_roots<LN, T, W>), dim3(wgs), dim3(T), 0, st, poly, occ, counts, n_work, grid, cosets, tabs, modmap, step, pts, g, rows, vrows, hits, found, hstride); break;
    switch (logn) {
        BR_CASE(13, 512, 4) BR_CASE(12, 256, 2) BR_CASE(6, 64, 4)
        default: throw_hip(hipErrorInvalidValue, __FILE__, __LINE__);
    }
#undef BR_CASE
    KERNEL_CHECK();
}

void launch_roots_gather(const u64 *poly, size_t n, const u32 *occ, const u32 *counts, u32 nrows, u64 c, Mod t, u64 *rows, hipStream_t st)
{
    if (!nrows) return;
    hipLaunchKernelGGL(k_roots_gather, dim3((unsigned)((n + EW_T - 1) / EW_T), nrows), dim3(EW_T), 0, st, poly, n, occ, counts, c, t, rows);
    KERNEL_CHECK();
}

void launch_roots_scan(const u64 *rows, size_t n, u32 nrows, const u64 *pts, u64 c, Mod t, bool first, const u64 *poly, const u32 *occ, const u32 *counts,
                       u64 *hits, u32 *found, u32 hstride, hipStream_t st)
{
    if (!nrows) return;
    hipLaunchKernelGGL(k_roots_scan, dim3((unsigned)((n + EW_T - 1) / EW_T), nrows), dim3(EW_T), 0, st, rows, n, pts, c, t, first ? 1 : 0, poly, occ, counts,
                       hits, found, hstride);
    KERNEL_CHECK();
}

void launch_roots_mult(u64 *poly, size_t n, const u32 *occ, const u32 *counts, u32 n_occ, Mod t, const u64 *hits, const u32 *found, u32 *mult, u32 hstride,
                       hipStream_t st)
{
    if (!n_occ) return;
    hipLaunchKernelGGL(k_roots_mult, dim3((n_occ + 3) / 4), dim3(256), 0, st, poly, n, occ, counts, n_occ, t, hits, found, mult, hstride);
    KERNEL_CHECK();
}

void launch_roots_split(const u64 *hits, const u32 *found, const u32 *mult, u32 hstride, const u32 *occ, const u32 *counts, u32 n_occ, u32 k, u64 *out,
                        const u64 *part_off, const u32 *part_stride, u32 *counts_out, u32 cstride, u64 *failure, hipStream_t st)
{
    const u32 cap = split_capacity(hstride);
    if (!k || !cap) throw_hip(hipErrorInvalidValue, __FILE__, __LINE__);
    { hipError_t e_ = hipMemsetAsync(counts_out, 0, (size_t)k * cstride * sizeof(u32), st); if (e_ != hipSuccess) throw_hip(e_, __FILE__, __LINE__); }
    if (!n_occ) return;
#define RS_CASE(CAP) case CAP: hipLaunchKernelGGL((k_roots_split<CAP, CAP == SPLIT_CAP_SMALL ? 64 : CAP == SPLIT_CAP_MID ? 256 : 1024>), dim3(n_occ), dim3(split_threads(CAP)), 0, st, hits, found, mult, hstride, occ, counts, k, out, part_off, part_stride, counts_out, cstride, reinterpret_cast<unsigned long long *>(failure)); break;
    switch (cap) {
        RS_CASE(SPLIT_CAP_SMALL) RS_CASE(SPLIT_CAP_MID) RS_CASE(SPLIT_CAP_LARGE)
    }
#undef RS_CASE
    KERNEL_CHECK();
}

void launch_bins_rows(const u64 *poly, size_t n, u32 rows, const u32 *counts, const u64 *off, const int *tops, u32 bins, u64 *out, hipStream_t st)
{
    if (!bins || !rows) return;
    hipLaunchKernelGGL(k_bins_rows, dim3((unsigned)((n + ROWS_TILE - 1) / ROWS_TILE), (rows + ROWS_TILE - 1) / ROWS_TILE), dim3(ROWS_TILE * ROWS_WAVES), 0, st,
                       poly, n, rows, counts, off, tops, bins, out);
    KERNEL_CHECK();
}

void launch_bins_eval(const u64 *poly, size_t n, u32 rows, const u32 *counts, const u64 *x, const u64 *mask, Mod t, u64 *out, unsigned char *is_bin, u32 *bad, hipStream_t st)
{
    if (!n || !rows) return;
    const dim3 grid((unsigned)((n + EVAL_LANES - 1) / EVAL_LANES));
    if (merge_narrow(merge_bits(t.q))) hipLaunchKernelGGL((k_bins_eval<true>), grid, dim3(EVAL_LANES), 0, st, poly, n, rows, counts, x, mask, t, out, is_bin, bad);
    else hipLaunchKernelGGL((k_bins_eval<false>), grid, dim3(EVAL_LANES), 0, st, poly, n, rows, counts, x, mask, t, out, is_bin, bad);
    KERNEL_CHECK();
}

void launch_eval_compare(const u64 *got, const u64 *want, size_t n, u32 count, u64 *status, hipStream_t st)
{
    if (!n || !count) return;
    hipLaunchKernelGGL(k_eval_compare, dim3((unsigned)((n + EW_T - 1) / EW_T), count), dim3(EW_T), 0, st, got, want, n, reinterpret_cast<unsigned long long *>(status));
    KERNEL_CHECK();
}

}  // namespace apsu_he
