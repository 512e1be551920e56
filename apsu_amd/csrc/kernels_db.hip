// The resident-database kernels of the query-evaluation engine for gfx950: BinBundle build (polyn_with_roots), update, find and place,
// merge, BatchEncoder's slot scatter and gather, algebraize, the entries' scatter and the PEQT block packing.  Rules and lane arithmetic:
// bin_update.h, bin_lookup.h, bin_merge.h, bulk_place.h, which the CPU tier runs as well.  (Reading the bins back: kernels_roots.hip.)
#include "launch_db.h"
#include "kernel_launch.h"
#include "bin_update.h"
#include "bin_lookup.h"
#include "bin_merge.h"
#include "bulk_place.h"
#include "mac_core.h"
#include <stdexcept>
#include <type_traits>

namespace apsu_he {

// ============================================================================ N1: BinBundle build on the GPU
// polyn_with_roots (common/apsu/util/interpolate.cpp:27-80) for every bin of a BinBundle.  One WAVE per bin: the
// monic polynomial lives in registers, coefficient i in lane i % 64, slot i / 64, so multiplying by (x - a) is one
// multiply-add per held coefficient plus a one-lane shift (P'[i] = P[i-1] - a P[i]); only the slots that can be
// non-zero after r roots are touched.  No LDS, no barriers.  Results are written column-wise ([degree][slot]); the
// buffer is zeroed beforehand, so bins beyond `bins` and degrees beyond a bin's count hold 0
// (BatchedPlaintextPolyn ctor, bin_bundle.cpp:395-405).
template <int SLOTS>
__global__ __launch_bounds__(256) void k_polyn_with_roots(const u64 *__restrict__ roots, const u32 *__restrict__ counts,
                                                          u32 bins, u32 stride, Mod t, u64 *__restrict__ poly, size_t n)
{
    const u32 lane = threadIdx.x & 63;
    const u32 s = blockIdx.x * 4 + (threadIdx.x >> 6);           // bin of this wave
    if (s >= bins) return;
    const u32 cnt = counts[s];
    u64 P[SLOTS];
#pragma unroll
    for (int j = 0; j < SLOTS; j++) P[j] = 0;
    if (lane == 0) P[0] = 1;
    const u64 *rt = roots + (size_t)s * stride;
    for (u32 r = 0; r < cnt; r++) {
        const u64 a = rt[r];
        const u64 neg_a = a ? t.q - a : 0;
        const int jmax = (int)((r + 1) >> 6);                    // highest slot holding a coefficient of degree <= r + 1
#pragma unroll
        for (int j = SLOTS - 1; j >= 0; j--) {
            if (j > jmax) continue;                              // wave-uniform
            u64 prev = __shfl_up((unsigned long long)P[j], 1, 64);                       // P[i-1] of the lane below
            const u64 wrap = j > 0 ? (u64)__shfl((unsigned long long)P[j > 0 ? j - 1 : 0], 63, 64) : 0;   // lane 0: last lane of slot j-1
            if (lane == 0) prev = wrap;
            P[j] = addmod(mulmod(P[j], neg_a, t), prev, t.q);
        }
    }
#pragma unroll
    for (int j = 0; j < SLOTS; j++) {
        const u32 d = (u32)j * 64 + lane;
        if (d <= cnt) poly[(size_t)d * n + s] = P[j];
    }
}

// fallback for polynomials beyond the largest wave-per-bin instance (more than 8192 coefficients): one thread per bin,
// coefficients in global memory
__global__ __launch_bounds__(EW_T) void k_polyn_with_roots_serial(const u64 *__restrict__ roots, const u32 *__restrict__ counts,
                                                                  u32 bins, u32 stride, Mod t, u64 *__restrict__ poly, size_t n)
{
    const size_t s = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (s >= bins) return;
    u64 *P = poly + s;                                          // P[d * n], zeroed by the caller
    const u32 cnt = counts[s];
    P[0] = 1;
    for (u32 r = 0; r < cnt; r++) {
        const u64 a = roots[(size_t)s * stride + r];
        const u64 neg_a = a ? t.q - a : 0;
        for (u32 i = r + 1; i > 0; i--)
            P[(size_t)i * n] = addmod(mulmod(P[(size_t)i * n], neg_a, t), P[(size_t)(i - 1) * n], t.q);
        P[0] = mulmod(P[0], neg_a, t);
    }
}

void launch_polyn_with_roots(const u64 *roots, const u32 *counts, u32 bins, u32 stride, u32 max_deg, Mod t, u64 *poly, size_t n,
                             hipStream_t st)
{
    { hipError_t e_ = hipMemsetAsync(poly, 0, (size_t)(max_deg + 1) * n * sizeof(u64), st); if (e_ != hipSuccess) throw_hip(e_, __FILE__, __LINE__); }
    if (!bins) return;
    const u32 slots = max_deg / 64 + 1;
    const dim3 g((bins + 3) / 4), b(256);
#define PW_CASE(S) if (slots <= S) { hipLaunchKernelGGL((k_polyn_with_roots<S>), g, b, 0, st, roots, counts, bins, stride, t, poly, n); KERNEL_CHECK(); return; }
    PW_CASE(1) PW_CASE(2) PW_CASE(4) PW_CASE(8) PW_CASE(16) PW_CASE(24) PW_CASE(32) PW_CASE(48) PW_CASE(64) PW_CASE(96) PW_CASE(128)
#undef PW_CASE
    hipLaunchKernelGGL(k_polyn_with_roots_serial, dim3((bins + EW_T - 1) / EW_T), dim3(EW_T), 0, st, roots, counts, bins, stride, t, poly, n);
    KERNEL_CHECK();
}

// ---- BinBundle update (Engine::update_bundle): insert / remove items of single bins of a resident BinBundle
// Decode, first step: limb 0 (the residues mod q_0) of `count` stored plaintext slots -> out[slot][n].  Dense slots are [L][n]
// words, bit-packed ones (k_pack_rows) hold mac_bits[0] bits per coefficient at the start of the slot.
__global__ __launch_bounds__(EW_T) void k_limb0_rows(const DevLevel *__restrict__ lv, int L, const char *__restrict__ src, size_t slot_bytes, int packed,
                                                     u64 *__restrict__ out, size_t n)
{
    const size_t c = (size_t)blockIdx.x * EW_T + threadIdx.x, slot = blockIdx.y;
    if (c >= n) return;
    u64 v;
    if (packed) {
        const u32 w = lv->mac_bits[0];
        v = packed_coeff(reinterpret_cast<const u32 *>(src + slot * slot_bytes + lv->mac_row_off[0]), c, w);   // (mac_core.h)
    } else v = reinterpret_cast<const u64 *>(src)[slot * (size_t)L * n + c];
    out[slot * n + c] = v;
}

void launch_limb0_rows(const DevLevel *lv, int L, const void *src, size_t slot_bytes, bool packed, u64 *out, size_t n, size_t count, hipStream_t st)
{
    if (!count) return;
    hipLaunchKernelGGL(k_limb0_rows, ew_grid(n, (int)count), dim3(EW_T), 0, st, lv, L, static_cast<const char *>(src), slot_bytes, packed ? 1 : 0, out, n);
    KERNEL_CHECK();
}

// Decode, after the inverse NTT over q_0: residues mod q_0 back to values mod t (bin_update.h)
__global__ __launch_bounds__(EW_T) void k_unlift(u64 *__restrict__ x, size_t words, u64 t, u64 q0)
{
    const size_t i = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (i < words) x[i] = bin_unlift(x[i], t, q0);
}

void launch_unlift(u64 *x, size_t words, u64 t, u64 q0, hipStream_t st)
{
    if (!words) return;
    hipLaunchKernelGGL(k_unlift, dim3((unsigned)((words + EW_T - 1) / EW_T)), dim3(EW_T), 0, st, x, words, t, q0);
    KERNEL_CHECK();
}

// one removal, register slots J .. 0 (top down).  Written as a recursion over the slot index so that every P[J] is a register whatever
// the unroller's size limits make of a loop this long (as a loop, the instances of 24 slots and more kept P in scratch memory).
template <int J, int SLOTS>
__device__ __forceinline__ void bins_remove_slots(u64 (&P)[SLOTS], u64 a, int jmax, u32 lane, u64 &carry, const Mod &t)
{
    if constexpr (J >= 0) {
        if (J <= jmax) {                                          // wave-uniform
            ScanPair p{ a, P[J] };
#pragma unroll 1
            for (int o = 1; o < 64; o <<= 1) {
                ScanPair up;
                up.m = __shfl_down((unsigned long long)p.m, o, 64);
                up.v = __shfl_down((unsigned long long)p.v, o, 64);
                if (lane + o < 64) p = bin_scan_compose(p, up, t);
            }
            const u64 sv = bin_scan_carry(p, carry, t);           // s_{64 J + lane}
            u64 q = __shfl_down((unsigned long long)sv, 1, 64);   // q_{k-1} = s_k: one lane down
            if (lane == 63) q = carry;
            P[J] = q;
            carry = __shfl((unsigned long long)sv, 0, 64);
        }
        bins_remove_slots<J - 1, SLOTS>(P, a, jmax, lane, carry, t);
    }
}

// P <- P / prod (x - rem_r) * prod (x - ins_r) for the bins named in `touched`, one WAVE per bin, on the columns of poly[rows][n]
// (slot values of the batched polynomial; other columns are not visited).  Register layout and insertion step of
// k_polyn_with_roots; the removal is synthetic division as a wave-level suffix scan (bin_update.h).  A bin's count is the index of its
// highest non-zero coefficient.  status[0]: atomicMin of (bin << 32 | position in the removal list) over the roots that left a
// remainder; status[1]: atomicMin of the bins named whose column is the zero polynomial (an unused slot).  Such a wave stops there.
// counts_out[w] = the new count of touched[w].  rows <= 64 * SLOTS; a bin never outgrows `rows` - 1 (the host sizes it).
template <int SLOTS>
__global__ __launch_bounds__(256) void k_bins_update(const u32 *__restrict__ touched, u32 n_touched,
                                                     const u64 *__restrict__ ins, const u32 *__restrict__ ins_counts, u32 ins_stride,
                                                     const u64 *__restrict__ rem, const u32 *__restrict__ rem_counts, u32 rem_stride,
                                                     Mod t, u64 *__restrict__ poly, size_t n, u32 rows, u32 *__restrict__ counts_out,
                                                     unsigned long long *__restrict__ status)
{
    const u32 lane = threadIdx.x & 63;
    const u32 w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_touched) return;
    const u32 s = touched[w];
    u64 P[SLOTS];
    int top = -1;                                                 // highest index of a non-zero coefficient in this lane
#pragma unroll
    for (int j = 0; j < SLOTS; j++) {
        const u32 d = (u32)j * 64 + lane;
        P[j] = d < rows ? poly[(size_t)d * n + s] : 0;
        if (P[j]) top = (int)d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o, 64));
    if (top < 0) {
        if (lane == 0) atomicMin(status + 1, (unsigned long long)s);
        return;
    }
    u32 cnt = (u32)top;
    const u32 n_rem = rem_counts ? rem_counts[s] : 0, n_ins = ins_counts ? ins_counts[s] : 0;
    for (u32 r = 0; r < n_rem; r++) {
        const u64 a = rem[(size_t)s * rem_stride + r];
        const int jmax = (int)(cnt >> 6);
        u64 carry = 0;                                            // s at lane 0 of the slot above
        if constexpr (SLOTS <= 32) bins_remove_slots<SLOTS - 1>(P, a, jmax, lane, carry, t);
        else {                                                    // (P lives in scratch memory in these instances anyway, as in the build)
#pragma unroll
            for (int j = SLOTS - 1; j >= 0; j--) {
                if (j > jmax) continue;                           // wave-uniform
                bins_remove_slots<0, 1>(reinterpret_cast<u64 (&)[1]>(P[j]), a, 0, lane, carry, t);
            }
        }
        if (carry != 0) {                                         // the remainder s_0
            if (lane == 0) atomicMin(status, (unsigned long long)bin_fail_word(s, r));
            return;
        }
        cnt--;
    }
    for (u32 r = 0; r < n_ins; r++) {
        const u64 a = ins[(size_t)s * ins_stride + r];
        const u64 neg_a = a ? t.q - a : 0;
        const int jmax = (int)((cnt + 1) >> 6);
#pragma unroll
        for (int j = SLOTS - 1; j >= 0; j--) {
            if (j > jmax) continue;
            u64 prev = __shfl_up((unsigned long long)P[j], 1, 64);
            const u64 wrap = j > 0 ? (u64)__shfl((unsigned long long)P[j > 0 ? j - 1 : 0], 63, 64) : 0;
            if (lane == 0) prev = wrap;
            P[j] = bin_insert_step(P[j], prev, neg_a, t);
        }
        cnt++;
    }
#pragma unroll
    for (int j = 0; j < SLOTS; j++) {
        const u32 d = (u32)j * 64 + lane;
        if (d < rows) poly[(size_t)d * n + s] = P[j];             // zero above the new count
    }
    if (lane == 0) counts_out[w] = cnt;
}

// the same beyond the largest wave-per-bin instance: one thread per bin, coefficients stay in global memory
__global__ __launch_bounds__(EW_T) void k_bins_update_serial(const u32 *__restrict__ touched, u32 n_touched,
                                                             const u64 *__restrict__ ins, const u32 *__restrict__ ins_counts, u32 ins_stride,
                                                             const u64 *__restrict__ rem, const u32 *__restrict__ rem_counts, u32 rem_stride,
                                                             Mod t, u64 *__restrict__ poly, size_t n, u32 rows, u32 *__restrict__ counts_out,
                                                             unsigned long long *__restrict__ status)
{
    const u32 w = blockIdx.x * EW_T + threadIdx.x;
    if (w >= n_touched) return;
    const u32 s = touched[w];
    u64 *P = poly + s;                                            // P[d * n]
    int top = (int)rows - 1;
    while (top >= 0 && P[(size_t)top * n] == 0) top--;
    if (top < 0) { atomicMin(status + 1, (unsigned long long)s); return; }
    u32 cnt = (u32)top;
    const u32 n_rem = rem_counts ? rem_counts[s] : 0, n_ins = ins_counts ? ins_counts[s] : 0;
    for (u32 r = 0; r < n_rem; r++) {
        const u64 a = rem[(size_t)s * rem_stride + r];
        u64 sv = 0;                                               // s_{k+1}
        for (int k = (int)cnt; k >= 0; k--) {
            const u64 pk = P[(size_t)k * n];
            P[(size_t)k * n] = sv;                                // q_k = s_{k+1}
            sv = addmod(pk, mulmod(a, sv, t), t.q);
        }
        if (sv != 0) { atomicMin(status, (unsigned long long)bin_fail_word(s, r)); return; }
        cnt--;
    }
    for (u32 r = 0; r < n_ins; r++) {
        const u64 a = ins[(size_t)s * ins_stride + r];
        const u64 neg_a = a ? t.q - a : 0;
        for (u32 i = cnt + 1; i > 0; i--) P[(size_t)i * n] = bin_insert_step(P[(size_t)i * n], P[(size_t)(i - 1) * n], neg_a, t);
        P[0] = mulmod(P[0], neg_a, t);
        cnt++;
    }
    counts_out[w] = cnt;
}

void launch_bins_update(const u32 *touched, u32 n_touched, const u64 *ins, const u32 *ins_counts, u32 ins_stride, const u64 *rem,
                        const u32 *rem_counts, u32 rem_stride, Mod t, u64 *poly, size_t n, u32 rows, u32 *counts_out, u64 *status, hipStream_t st)
{
    if (!n_touched) return;
    unsigned long long *stw = reinterpret_cast<unsigned long long *>(status);
    const u32 slots = (rows + 63) / 64;
    const dim3 g((n_touched + 3) / 4), b(256);
#define BU_CASE(S) if (slots <= S) { hipLaunchKernelGGL((k_bins_update<S>), g, b, 0, st, touched, n_touched, ins, ins_counts, ins_stride, rem, rem_counts, rem_stride, t, poly, n, rows, counts_out, stw); KERNEL_CHECK(); return; }
    BU_CASE(1) BU_CASE(2) BU_CASE(4) BU_CASE(8) BU_CASE(16) BU_CASE(24) BU_CASE(32) BU_CASE(48) BU_CASE(64) BU_CASE(96) BU_CASE(128)
#undef BU_CASE
    hipLaunchKernelGGL(k_bins_update_serial, dim3((n_touched + EW_T - 1) / EW_T), dim3(EW_T), 0, st, touched, n_touched, ins, ins_counts, ins_stride,
                       rem, rem_counts, rem_stride, t, poly, n, rows, counts_out, stw);
    KERNEL_CHECK();
}

// the degree of the batched polynomial: atomicMax over the slots of the index of the highest non-zero row of poly[rows][n]
__global__ __launch_bounds__(EW_T) void k_poly_degree(const u64 *__restrict__ poly, size_t n, u32 rows, unsigned long long *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    int top = (int)rows - 1;
    while (top > 0 && poly[(size_t)top * n + i] == 0) top--;
    if (top > 0) atomicMax(out, (unsigned long long)top);
}

void launch_poly_degree(const u64 *poly, size_t n, u32 rows, u64 *out, hipStream_t st)
{
    hipLaunchKernelGGL(k_poly_degree, dim3((unsigned)((n + EW_T - 1) / EW_T)), dim3(EW_T), 0, st, poly, n, rows, reinterpret_cast<unsigned long long *>(out));
    KERNEL_CHECK();
}

// ---- find and place (Engine::lookup_bundles): questions to the decoded poly[rows][n] of a resident BinBundle (bin_lookup.h)
// counts[slot] = index of the highest non-zero coefficient of the slot's polynomial, LOOKUP_NONE for the zero polynomial (not a bin).
// One lane per slot, rows walked from the top: a wave reads a contiguous row segment, and stops at the first row in a full bin.
__global__ __launch_bounds__(EW_T) void k_bin_counts(const u64 *__restrict__ poly, size_t n, u32 rows, u32 *__restrict__ counts)
{
    const size_t i = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    int top = (int)rows - 1;
    while (top >= 0 && poly[(size_t)top * n + i] == 0) top--;
    counts[i] = bin_count_of(top);
}

void launch_bin_counts(const u64 *poly, size_t n, u32 rows, u32 *counts, hipStream_t st)
{
    hipLaunchKernelGGL(k_bin_counts, dim3((unsigned)((n + EW_T - 1) / EW_T)), dim3(EW_T), 0, st, poly, n, rows, counts);
    KERNEL_CHECK();
}

// Horner evaluation of the bins' polynomials at the entries' parts.  Lane = slot: one WAVE per work item (tile of 64 consecutive slots,
// up to R rows of points: lookup_plan), rows d = degree .. 0 with one contiguous 512-byte segment per d and R independent
// acc = acc x + p steps per lane, so every stored coefficient is read once per R points of its tile and no lane walks down a column.
// The rows are taken four at a time, loads first, so that four segments are in flight per wave.  flags[part] = 1 iff the point is a
// root and the slot is a bin (lookup_found); every part is written by exactly one lane.  No LDS.
template <int R>
__global__ __launch_bounds__(256) void k_bins_lookup(const LookupWork *__restrict__ work, u32 n_work, const u64 *__restrict__ pts,
                                                     const u32 *__restrict__ idx, Mod t, const u64 *__restrict__ poly, size_t n, u32 degree,
                                                     unsigned char *__restrict__ flags)
{
    const u32 lane = threadIdx.x & 63;
    const u32 w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_work) return;
    const LookupWork wk = work[w];
    const size_t slot = (size_t)wk.tile * LOOKUP_LANES + lane;
    const bool live = slot < n;                                   // (n < 64 only)
    const u64 *col = poly + (live ? slot : 0);
    u64 x[R], acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        x[r] = (u32)r < wk.nrows ? pts[((size_t)wk.row0 + r) * LOOKUP_LANES + lane] : 0;
        acc[r] = 0;
    }
    u64 nz = 0;
    int d = (int)degree;
    for (; d >= 3; d -= 4) {
        u64 p[4];
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = col[(size_t)(d - k) * n];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            nz |= p[k];
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = lookup_horner_step(acc[r], x[r], p[k], t);
        }
    }
    for (; d >= 0; d--) {
        const u64 p = col[(size_t)d * n];
        nz |= p;
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = lookup_horner_step(acc[r], x[r], p, t);
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        if ((u32)r >= wk.nrows) break;
        const u32 part = idx[((size_t)wk.row0 + r) * LOOKUP_LANES + lane];
        if (part != LOOKUP_NONE) flags[part] = live && lookup_found(acc[r], nz) ? 1 : 0;
    }
}

void launch_bins_lookup(const LookupWork *work, u32 n_work, const u64 *pts, const u32 *idx, Mod t, const u64 *poly, size_t n, u32 degree,
                        unsigned char *flags, hipStream_t st)
{
    if (!n_work) return;
    hipLaunchKernelGGL((k_bins_lookup<LOOKUP_R>), dim3((n_work + 3) / 4), dim3(256), 0, st, work, n_work, pts, idx, t, poly, n, degree, flags);
    KERNEL_CHECK();
}

// ---- merge (Engine::merge_bundles): the per-slot product of two decoded BinBundles, C[k] = sum_{i+j=k} A[i] B[j] mod t (bin_merge.h)
// Lane = slot: one WAVE per (tile of 64 consecutive slots, block of K = MERGE_K consecutive output rows), the K sums in registers.
// The wave walks A's rows i; a step takes the contiguous row segment A[i] and ONE new row B[k0 - i] of the K-row window of B that
// slides with it, and does K multiply-adds, so no lane walks down a column and every row segment is read once per K output rows.
// The walk is unrolled K times from a multiple of K, which turns the window's shift into compile-time slot numbers, and the 2 K row
// loads of a chunk are issued before its K K multiply-adds.  Rows outside 0 .. top read the nearest row inside (no branch, no
// out-of-range address) and count as 0.  tops: the tile's largest counts (-1: no bin), which bound the walk.  NARROW (t < 2^32):
// operands are the low words, the sums 64-bit (v_mad_u64_u32); otherwise 128-bit sums.  `fold` steps between two reductions
// (merge_fold_interval).  Every row k < rows of C is written for every slot.  No LDS.
template <bool NARROW>
__global__ __launch_bounds__(256) void k_bins_merge(const u64 *__restrict__ A, const int *__restrict__ topsA, const u64 *__restrict__ B,
                                                    const int *__restrict__ topsB, Mod t, u32 fold, u64 *__restrict__ C, size_t n, u32 rows,
                                                    u32 blocks, u32 n_work)
{
    constexpr int K = MERGE_K;
    using Acc = typename std::conditional<NARROW, u64, u128p>::type;
    using Val = typename std::conditional<NARROW, u32, u64>::type;
    const u32 lane = threadIdx.x & 63;
    const u32 w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (w >= n_work) return;
    const u32 tile = w / blocks;
    const int k0 = (int)(w % blocks) * K;
    const size_t slot = (size_t)tile * MERGE_LANES + lane;
    const bool live = slot < n;                                   // (n < 64 only)
    const u64 *colA = A + (live ? slot : 0), *colB = B + (live ? slot : 0);
    const int topA = __builtin_amdgcn_readfirstlane(topsA[tile]), topB = __builtin_amdgcn_readfirstlane(topsB[tile]);
    const MergeWalk wk = merge_walk(k0, K, topA, topB);
    Acc acc[K];
#pragma unroll
    for (int j = 0; j < K; j++) acc[j] = Acc{};
    if (wk.i1 >= wk.i0) {                                         // (then topA >= 0 and topB >= 0)
        // a row of B, 0 outside 0 .. topB; of A, 0 beyond the walk's last step
        auto rowB = [&](int r) -> Val {
            const int rc = r < 0 ? 0 : (r > topB ? topB : r);
            const Val v = (Val)colB[(size_t)rc * n];
            return r == rc ? v : (Val)0;
        };
        auto rowA = [&](int i) -> Val {
            const Val v = (Val)colA[(size_t)(i > wk.i1 ? wk.i1 : i) * n];
            return i <= wk.i1 ? v : (Val)0;
        };
        Val win[K];
        win[0] = 0;
#pragma unroll
        for (int j = 1; j < K; j++) win[j] = rowB(k0 - wk.i0 + j);
        u32 pending = 0;
        for (int ib = wk.i0; ib <= wk.i1; ib += K) {
            Val a[K], nb[K];
#pragma unroll
            for (int u = 0; u < K; u++) {
                a[u] = rowA(ib + u);
                nb[u] = rowB(k0 - ib - u);
            }
#pragma unroll
            for (int u = 0; u < K; u++) {
                if (pending == fold) {                            // wave-uniform
#pragma unroll
                    for (int j = 0; j < K; j++) {
                        if constexpr (NARROW) acc[j] = merge_fold_narrow(acc[j], t);
                        else acc[j] = u128p{ merge_fold_wide(acc[j], t), 0 };
                    }
                    pending = 0;
                }
                pending++;
                win[(K - u) % K] = nb[u];
#pragma unroll
                for (int j = 0; j < K; j++) {
                    if constexpr (NARROW) merge_mac_narrow(acc[j], a[u], win[(j - u + K) % K]);
                    else merge_mac_wide(acc[j], a[u], win[(j - u + K) % K]);
                }
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int j = 0; j < K; j++) {
        if ((u32)(k0 + j) >= rows) break;
        if constexpr (NARROW) C[(size_t)(k0 + j) * n + slot] = merge_fold_narrow(acc[j], t);
        else C[(size_t)(k0 + j) * n + slot] = merge_fold_wide(acc[j], t);
    }
}

void launch_bins_merge(const u64 *A, const int *topsA, const u64 *B, const int *topsB, Mod t, u64 *C, size_t n, u32 rows, hipStream_t st)
{
    const int bits = merge_bits(t.q);
    const u64 tiles = (n + MERGE_LANES - 1) / MERGE_LANES, blocks = ((u64)rows + MERGE_K - 1) / MERGE_K, n_work = tiles * blocks;
    if (!n_work) return;
    if (n_work > 0x7fffffffu) throw std::invalid_argument("merge: too many rows for one launch");
    const dim3 g((unsigned)((n_work + 3) / 4)), b(256);
    if (merge_narrow(bits))
        hipLaunchKernelGGL((k_bins_merge<true>), g, b, 0, st, A, topsA, B, topsB, t, merge_fold_interval(bits), C, n, rows, (u32)blocks, (u32)n_work);
    else
        hipLaunchKernelGGL((k_bins_merge<false>), g, b, 0, st, A, topsA, B, topsB, t, merge_fold_interval(bits), C, n, rows, (u32)blocks, (u32)n_work);
    KERNEL_CHECK();
}

// BatchEncoder::encode, first half (App. B4): out[b][slot_map[i]] = in[b][i]; the inverse NTT mod t follows
__global__ __launch_bounds__(EW_T) void k_scatter_slots(const u64 *__restrict__ in, const u32 *__restrict__ slot_map,
                                                        u64 *__restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const size_t b = blockIdx.y;
    out[b * n + slot_map[i]] = in[b * n + i];
}

void launch_scatter_slots(const u64 *in, const u32 *slot_map, u64 *out, size_t n, int batch, hipStream_t st)
{
    if (!batch) return;
    hipLaunchKernelGGL(k_scatter_slots, ew_grid(n, batch), dim3(EW_T), 0, st, in, slot_map, out, n);
    KERNEL_CHECK();
}

// BatchEncoder::decode's slot gather (after the forward NTT mod t): out[b][i] = in[b][slot_map[i]]
__global__ __launch_bounds__(EW_T) void k_gather_slots(const u64 *__restrict__ in, const u32 *__restrict__ slot_map,
                                                       u64 *__restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const size_t b = blockIdx.y;
    out[b * n + i] = in[b * n + slot_map[i]];
}

void launch_gather_slots(const u64 *in, const u32 *slot_map, u64 *out, size_t n, int batch, hipStream_t st)
{
    if (!batch) return;
    hipLaunchKernelGGL(k_gather_slots, ew_grid(n, batch), dim3(EW_T), 0, st, in, slot_map, out, n);
    KERNEL_CHECK();
}

// N1: algebraize_item (common/apsu/util/db_encoding.cpp:209-256,360-366): felt j of an item = bits [j*bpf, j*bpf + bpf) of its
// first item_bits bits, the item read as a little-endian bit string (bit k = bit k%8 of byte k/8); one thread per felt
__global__ __launch_bounds__(EW_T) void k_algebraize(const unsigned char *__restrict__ items, size_t count, u32 felts, u32 bpf, u32 item_bits,
                                                     u64 *__restrict__ out)
{
    const size_t idx = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (idx >= count * felts) return;
    const size_t it = idx / felts;
    const u32 j = (u32)(idx % felts);
    const unsigned char *p = items + it * 16;
    u64 lo = 0, hi = 0;
#pragma unroll
    for (int b = 0; b < 8; b++) { lo |= (u64)p[b] << (8 * b); hi |= (u64)p[8 + b] << (8 * b); }
    const u32 off = j * bpf;
    const u32 take = off >= item_bits ? 0 : (item_bits - off < bpf ? item_bits - off : bpf);
    u64 v = off >= 64 ? hi >> (off - 64) : (off ? (lo >> off) | (hi << (64 - off)) : lo);
    out[idx] = take ? v & (~(u64)0 >> (64 - take)) : 0;
}

void launch_algebraize(const unsigned char *items, size_t count, u32 felts, u32 bpf, u32 item_bits, u64 *out, hipStream_t st)
{
    if (!count) return;
    hipLaunchKernelGGL(k_algebraize, dim3((unsigned)((count * felts + EW_T - 1) / EW_T)), dim3(EW_T), 0, st, items, count, felts, bpf, item_bits, out);
    KERNEL_CHECK();
}

// N1, a whole database from its entries (Engine::build_from_entries; bulk_place.h): the root lists of ONE target BinBundle (bundle
// index, k) straight from the bundle index's post-OPRF items -- a streaming transposition, 16 bytes in and 8 F bytes out per entry.
// Workgroup (location, block of entries): the lane is the entry (entries_scatter_lane).  Plain vector loads and stores: no atomics, no LDS.
__global__ __launch_bounds__(SCATTER_T) void k_entries_scatter(const BulkItem *__restrict__ items, const u64 *__restrict__ offsets,
                                                               const u32 *__restrict__ kstart, u32 locations, u32 F, u32 bpf, u32 item_bits, u32 cap,
                                                               u32 k, u32 stride, u64 *__restrict__ roots, u32 *__restrict__ counts, u32 n_counts)
{
    entries_scatter_lane(items, offsets, kstart, locations, F, bpf, item_bits, cap, k, stride, roots, counts, n_counts, blockIdx.x, blockIdx.y,
                         gridDim.y, threadIdx.x, SCATTER_T);
}

void launch_entries_scatter(const void *items, const u64 *offsets, const u32 *kstart, u32 locations, u32 F, u32 bpf, u32 item_bits, u32 cap, u32 k,
                            u32 stride, u64 *roots, u32 *counts, u32 n_counts, u32 blocks, hipStream_t st)
{
    if (!F || F > SCATTER_MAX_F || !bpf || bpf > 64 || (u64)(F - 1) * bpf >= 128) throw std::invalid_argument("entries_scatter: felts_per_item or bits per felt out of range");
    if (!cap || !stride || stride >= ((u32)1 << 30)) throw std::invalid_argument("entries_scatter: cap or stride out of range");
    if ((u64)locations * F > n_counts) throw std::invalid_argument("entries_scatter: more bins than count words");
    if ((uintptr_t)items & 15) throw std::invalid_argument("entries_scatter: the items are not 16-byte aligned");
    if (!blocks) blocks = scatter_blocks(locations, cap);
    if (blocks > 65535) throw std::invalid_argument("entries_scatter: more than 65535 workgroups per location");
    hipLaunchKernelGGL(k_entries_scatter, dim3(locations + 1, blocks), dim3(SCATTER_T), 0, st, static_cast<const BulkItem *>(items), offsets, kstart, locations,
                       F, bpf, item_bits, cap, k, stride, roots, counts, n_counts);
    KERNEL_CHECK();
}

// N4: vec_to_oc_block (receiver_osn.cpp:53-73): the felts of one item packed into a 128-bit block for the PEQT step,
// out[item] = (lower, higher).  len = bit length of the plain modulus as the reference computes it; the odd-felt
// branch shifts the upper half by len/2 - 1 (not len/2) exactly as the reference does; 64-bit shifts wrap.
__global__ __launch_bounds__(EW_T) void k_pack_blocks(const u64 *__restrict__ values, size_t n, u32 items, u32 felts, u32 len,
                                                      u64 *__restrict__ out)
{
    const size_t it = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (it >= items) return;
    const size_t b = blockIdx.y;
    const u64 *in = values + b * n + it * felts;
    const u64 mask = ((u64)1 << len) - 1, mask_lower = ((u64)1 << (len >> 1)) - 1, mask_higher = mask - mask_lower;
    u64 lower = 0, higher = 0;
    if (felts & 1) {
        lower = in[felts - 1] & mask_lower;
        higher = (in[felts - 1] & mask_higher) >> ((len >> 1) - 1);
    }
    for (u32 p = 0; p + 1 < felts; p += 2) {
        lower = (in[p] & mask) | (lower << len);
        higher = (in[p + 1] & mask) | (higher << len);
    }
    out[(b * items + it) * 2] = lower;
    out[(b * items + it) * 2 + 1] = higher;
}

void launch_pack_blocks(const u64 *values, size_t n, u32 items, u32 felts, u32 len, u64 *out, int batch, hipStream_t st)
{
    if (!batch || !items) return;
    hipLaunchKernelGGL(k_pack_blocks, ew_grid(items, batch), dim3(EW_T), 0, st, values, n, items, felts, len, out);
    KERNEL_CHECK();
}

} // namespace apsu_he
