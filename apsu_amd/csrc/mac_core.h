// The multiply-accumulate family's arithmetic, written once: the per-lane bodies of k_mac, k_term_product, k_pack_rows and
// k_unpack_rows (kernels_mac.hip), the bit-packed row extraction, and the rules for the operand split and the carry-free chunks.
// The gfx950 kernels run these functions and emu/mac.cpp steps the same functions over every lane of a grid on the CPU
// (tests/test_mac_core_cpu.py), as ntt_core.h does for the transforms.
#pragma once
#include <stddef.h>
#include "dev_consts.h"

namespace apsu_he {

constexpr int MAC_G = 4;                                          // streams per multiply-accumulate job
constexpr int MAC_C = 2;                                          // coefficients per lane (one 16-byte load)

// Multiply-accumulate job: for g < ng:  out[g][2][L][n] = sum_{j<cnt} PW_j (.) PT_{g,j}   (NTT domain).
// All streams of a job share the ciphertext powers PW (same bundle index) and the term count.
struct MacJob {
    const u64 *pt[MAC_G]; // first plaintext of stream g; term j at + j*pt_stride ; limb l at + l*n
    u64 *out[MAC_G];      // [2][L][n]
    const u64 *pw;        // first ciphertext; term j at pw + j*pw_stride ; poly p at + p*pw_poly_stride
    u32 cnt, ng;
    u32 pt_stride, pw_stride, pw_poly_stride;        // in u64 words
    u32 out_poly_stride;  // words between the two output polynomials (L*n for a full ciphertext)
    u32 limb0, nl;        // limbs limb0 .. limb0+nl-1 are handled (grid.y >= nl exits); modulus = q[limb]
    u32 packed, pad;      // packed: pt[] point at bit-packed plaintext slots and pt_stride is in BYTES (DevLevel::mac_bits); pad: reserved, 0
};
struct TermJob { const u64 *pt; const u64 *pw; u64 *out; };     // a single product on one limb (k_term_product); pt: the slot as k_mac takes it

// ---- the rules of the carry-free accumulation, as functions of the modulus (build_level fills DevLevel from them)
// Both operands are < q < 2^(2s), s = ceil(bits(q)/2) <= 30: each is split into two s-bit halves.
inline int mac_shift_of(u64 q) { return (64 - __builtin_clzll(q) + 1) / 2; }
// terms per chunk of the four-product form: the cross sum takes two products (< 2^(2s)) per term, plus one slot for the carried residue
inline u32 mac_chunk_of(u64 q)
{
    const u64 cap = (u64)1 << (63 - 2 * mac_shift_of(q)), c = cap > 2 ? cap - 1 : 2;
    return (u32)(c < (1u << 20) ? c : 1u << 20);
}
// ... of the three-product form: one middle product (a0 + a1)(c0 + c1) < 2^(2s + 2) per term, the carried residue enters as
// (r0, r0 + r1) < 2^(s + 1): one slot as well.  0: none.  (Conservative: the middle sum may wrap, Smid - S00 - S11 is taken mod 2^64.)
inline u32 mac_chunk_k_of(u64 q)
{
    const int s = mac_shift_of(q);
    const u64 capk = 2 * s + 2 < 64 ? (u64)1 << (62 - 2 * s) : 0, c = capk > 2 ? capk - 1 : 0;
    return (u32)(c < (1u << 20) ? c : 1u << 20);
}
// PACKED k_mac cuts the high half out of a w-bit coefficient with this mask (dense rows, w = 64: the shift alone leaves it clean)
inline u32 mac_mask_hi_of(u32 w, int s) { return w == 64 ? 0xffffffffu : (u32)(((u64)1 << (w - s)) - 1); }
// Can a launch over this modulus take the three-product form?  It needs carry-free chunks of at least 7 terms (62 - 2s >= 3):
// a 59- or 60-bit prime has 3 and is refused.
inline bool mac_kara_usable(u64 q) { return mac_chunk_k_of(q) >= 7; }

// Kept sums (round 4): an empty assembly statement on every partial sum of k_mac's inner loop.  Without it the compiler pairs two products
// first and adds the pair to the running sum with a separate 64-bit add; with it every product is ONE v_mad_u64_u32 whose addend is the sum:
// 283 instead of 315 VALU instructions per two terms, -2.2 % on the 16M-4096 query (profiles/r04_ab_mac_kept_sums.txt).  Device only.
#if defined(__HIP_DEVICE_COMPILE__)
#define MAC_KEEP(v) asm("" : "+v"(v))
#else
#define MAC_KEEP(v) do { } while (0)
#endif

HD u32 alignbit(u32 hi, u32 lo, u32 sh)                          // bits [sh, sh + 32) of hi:lo, sh < 32 (v_alignbit_b32)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, sh);
#else
    return (u32)((((u64)hi << 32) | lo) >> (sh & 31));
#endif
}

// ---- bit-packed rows: limb j of a stored plaintext takes kb = mac_bits[j] bits per coefficient.  Pair window: coefficients k, k + 1 (k even)
// occupy 2 kb bits from bit kb k of the row, i.e. inside the 16 bytes that start at the dword holding that bit (the host picks widths for
// which shift + 2 kb <= 128 everywhere).  Returns that dword; psh = the pair's bit offset inside it.
HD const u32 *packed_window(const void *slot, u32 row_off, size_t k, u32 kb, u32 &psh)
{
    const u32 bitoff = (u32)(k >> 1) * 2 * kb;
    psh = bitoff & 31;
    return reinterpret_cast<const u32 *>(static_cast<const char *>(slot) + row_off) + (bitoff >> 5);
}
// the window (w_lo: bytes 0-7, w_hi: bytes 8-15) shifted down by psh with funnel shifts: the pair then starts at bit 0 of lo:hi
HD void packed_shift(u64 w_lo, u64 w_hi, u32 psh, u64 &lo64, u64 &hi64)
{
    const u32 w0 = (u32)w_lo, w1 = (u32)(w_lo >> 32), w2 = (u32)w_hi, w3 = (u32)(w_hi >> 32);
    const u32 n0 = alignbit(w1, w0, psh), n1 = alignbit(w2, w1, psh), n2 = alignbit(w3, w2, psh), n3 = w3 >> psh;
    lo64 = (u64)n0 | ((u64)n1 << 32); hi64 = (u64)n2 | ((u64)n3 << 32);
}
// the second coefficient of a shifted window, bits [kb, 2 kb) of hi64:lo64 (the first: bits [0, kb) of lo64); what lies above is NOT cleared.
// A macro: as a function the compiler orders the OR's operands on its own and k_mac's instruction stream differs from the recorded one.
#define PACKED_SECOND(lo64, hi64, kb) ((kb) == 64 ? (hi64) : (((lo64) >> (kb)) | ((hi64) << (64 - (kb)))))
// coefficients k, k + 1 of a row from their window, clean
HD void packed_pair(u64 w_lo, u64 w_hi, u32 psh, u32 kb, u64 &a0, u64 &a1)
{
    u64 lo64, hi64;
    packed_shift(w_lo, w_hi, psh, lo64, hi64);
    if (kb == 64) { a0 = lo64; a1 = hi64; }
    else { const u64 mask = ((u64)1 << kb) - 1; a0 = lo64 & mask; a1 = PACKED_SECOND(lo64, hi64, kb) & mask; }
}
// one coefficient of a row of w-bit coefficients, by 4-byte reads (a packed buffer ends in 16 readable bytes: the engine pads)
HD u64 packed_coeff(const u32 *row, size_t c, u32 w)
{
    const size_t bit0 = c * w, d0 = bit0 >> 5;
    const u32 sh = (u32)(bit0 & 31);
    u64 v = ((u64)row[d0] | ((u64)row[d0 + 1] << 32)) >> sh;
    if (sh && w + sh > 64) v |= (u64)row[d0 + 2] << (64 - sh);
    return w == 64 ? v : (v & (((u64)1 << w) - 1));
}

// ---- k_mac, one lane (block indices bx, by, bz; thread tx).  For hipcc this function IS the kernel, not a body that a kernel calls: the
// compiler optimises a called body on its own before it inlines it, and k_mac's instruction stream then differs from the recorded one
// (operand order, block layout; profiles/r13_mac_core_refactor.txt), where no timing can tell whether that matters.  For a host compiler
// it is a plain function that takes the lane's position as arguments; emu/mac.cpp steps it over every lane of a grid.
#if defined(__HIPCC__)
#define MAC_LANE_FN __global__ __launch_bounds__(EW_T, 1) void
#define MAC_LANE_AT
#define MAC_LANE_AT_DEF const unsigned bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z, tx = threadIdx.x
#else
#define MAC_LANE_FN inline void
#define MAC_LANE_AT , unsigned bx, unsigned by, unsigned bz, unsigned tx
#define MAC_LANE_AT_DEF (void)0
#endif
// Carry-free accumulation: the three partial sums  S00 += lo*lo,  Sx += lo*hi + hi*lo,  S11 += hi*hi  of the s-bit operand halves are plain
// 64-bit v_mad_u64_u32 accumulations (no carries, no compares): 4 multiply-adds per product and nothing else.  `chunk` terms are accumulated
// before the sums are recombined (S00 + Sx*2^s + S11*2^(2s)) and reduced; for the 48..56-bit primes a whole inner polynomial fits in one chunk.
// KARA: three products per (stream, coefficient, polynomial, term) instead of four -- S00 += a0 c0, S11 += a1 c1, Smid += (a0 + a1)(c0 + c1),
// the cross sum recovered at fold time as Smid - S00 - S11; the power-side sums c0 + c1 are formed once per term and shared by the G streams.
// Its chunk is half as long (lv->mac_chunk_k); the carried residue r re-enters as the "term" (a0 c0, mid) = (r mod 2^s, r mod 2^s + (r >> s)).
// PACKED: still ONE 16-byte load per term and stream (packed_window, packed_shift): fewer HBM bytes per term, as many load instructions.
// Grid order (mac_grid, mac_plan.h).  Workgroups go to the XCDs round-robin in launch order, so what is FAST in the grid decides which
// workgroups are resident behind one L2 together, i.e. how much of the shared powers that L2 has to hold:
//   limb_slow 0: (block, limb, job)  -- an XCD holds blocks x, x + 8 of every limb of ~10 jobs: 2 * limbs * terms * 8 KiB
//   limb_slow 1: (block, job, limb)  -- ... of ONE limb of ~32 jobs: 2 * terms * 8 KiB  (profiles/r04_ab_mac_grid_order.txt)
template <bool KARA, bool PACKED>
MAC_LANE_FN k_mac(const DevLevel *__restrict__ lv, const MacJob *__restrict__ jobs, size_t n, int limb_slow MAC_LANE_AT)
{
    MAC_LANE_AT_DEF;
    constexpr int G = MAC_G, C = MAC_C;
    unsigned b_x = bx, b_limb = by, b_job = bz;
    if (limb_slow) { b_limb = bz; b_job = by; }
    const size_t k = ((size_t)b_x * EW_T + tx) * C;
    if (k >= n) return;
    const MacJob *__restrict__ jp = jobs + b_job;                // stream pointers are indexed dynamically: read them from memory
    struct { const u64 *pw; u32 cnt, ng, pt_stride, pw_stride, pw_poly_stride, out_poly_stride, limb0; } job =
        { jp->pw, jp->cnt, jp->ng, jp->pt_stride, jp->pw_stride, jp->pw_poly_stride, jp->out_poly_stride, jp->limb0 };
    if ((int)job.ng <= 0 || b_limb >= jp->nl) return;
    const int j = b_limb + job.limb0;                          // limb
    const Mod m = lv->q[j];
    const u32 s = lv->mac_shift[j], chunk = KARA ? lv->mac_chunk_k[j] : lv->mac_chunk[j];
    const u32 lomask = (1u << s) - 1;                          // s <= 30
    const u64 *p0 = job.pw + (size_t)j * n + k;
    const u64 *p1 = p0 + job.pw_poly_stride;
    const u64 *pt[G];
    const u32 *ptw[G];                                          // PACKED: first dword of this lane's 16-byte window
    u32 psh = 0, kb = 64, himask = 0xffffffffu;
    if constexpr (PACKED) {
        kb = lv->mac_bits[j];
        himask = lv->mac_mask_hi[j];
#pragma unroll
        for (int g = 0; g < G; g++) ptw[g] = packed_window(jp->pt[g < (int)job.ng ? g : 0], lv->mac_row_off[j], k, kb, psh);
    } else {
#pragma unroll
        for (int g = 0; g < G; g++) pt[g] = jp->pt[g < (int)job.ng ? g : 0] + (size_t)j * n + k;   // missing streams alias a real one
    }

    // accumulators [stream][coef][poly]
    u64 s00[G][C][2], sx[G][C][2], s11[G][C][2];
#pragma unroll
    for (int g = 0; g < G; g++)
#pragma unroll
        for (int c = 0; c < C; c++)
#pragma unroll
            for (int p = 0; p < 2; p++) s00[g][c][p] = sx[g][c][p] = s11[g][c][p] = 0;

    struct Term { u64 c[2][C]; u64 a[G][C]; };                  // powers (poly, coef) and plaintext values (stream, coef)
    auto load_term = [&](u32 i, Term &t) {
        const u64x2 v0 = ldg16(p0 + (size_t)i * job.pw_stride), v1 = ldg16(p1 + (size_t)i * job.pw_stride);
        t.c[0][0] = v0[0]; t.c[0][1] = v0[1]; t.c[1][0] = v1[0]; t.c[1][1] = v1[1];
#pragma unroll
        for (int g = 0; g < G; g++) {
            if constexpr (PACKED) {
                const u32x4a4 w = ldg16_a4_nt(ptw[g] + (size_t)i * (job.pt_stride >> 2));      // pt_stride in bytes
                t.a[g][0] = (u64)w[0] | ((u64)w[1] << 32); t.a[g][1] = (u64)w[2] | ((u64)w[3] << 32);
            } else {
                const u64x2 a = ldg16_nt(pt[g] + (size_t)i * job.pt_stride);
                t.a[g][0] = a[0]; t.a[g][1] = a[1];
            }
        }
    };
    auto mac_term = [&](const Term &t) {
        u32 clo[2][C], chi[2][C];
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int c = 0; c < C; c++) { clo[p][c] = (u32)t.c[p][c] & lomask; chi[p][c] = (u32)(t.c[p][c] >> s); }
        u32 csum[2][C];
        if (KARA) {
#pragma unroll
            for (int p = 0; p < 2; p++)
#pragma unroll
                for (int c = 0; c < C; c++) csum[p][c] = clo[p][c] + chi[p][c];
        }
#pragma unroll
        for (int g = 0; g < G; g++) {
            u64 av[C];
            if constexpr (PACKED) {
                u64 hi64;
                packed_shift(t.a[g][0], t.a[g][1], psh, av[0], hi64);
                av[1] = PACKED_SECOND(av[0], hi64, kb);                 // (lomask and himask clear what lies above)
            }
            else {
#pragma unroll
                for (int c = 0; c < C; c++) av[c] = t.a[g][c];
            }
#pragma unroll
            for (int c = 0; c < C; c++) {
                const u32 alo = (u32)av[c] & lomask, ahi = PACKED ? ((u32)(av[c] >> s) & himask) : (u32)(av[c] >> s);
#pragma unroll
                for (int p = 0; p < 2; p++) {
                    s00[g][c][p] += (u64)alo * clo[p][c]; MAC_KEEP(s00[g][c][p]);
                    if (KARA) { sx[g][c][p] += (u64)(alo + ahi) * csum[p][c]; MAC_KEEP(sx[g][c][p]); }
                    else {
                        sx[g][c][p] += (u64)alo * chi[p][c]; MAC_KEEP(sx[g][c][p]);
                        sx[g][c][p] += (u64)ahi * clo[p][c]; MAC_KEEP(sx[g][c][p]);
                    }
                    s11[g][c][p] += (u64)ahi * chi[p][c]; MAC_KEEP(s11[g][c][p]);
                }
            }
        }
    };
    // recombine S00 + Sx*2^s + S11*2^(2s) (< 2^128) and reduce; the residue re-enters as the next chunk's S00
    auto fold = [&](bool last) {
#pragma unroll
        for (int g = 0; g < G; g++)
#pragma unroll
            for (int c = 0; c < C; c++)
#pragma unroll
                for (int p = 0; p < 2; p++) {
                    u128p acc{ s00[g][c][p], 0 };
                    const u64 cross = KARA ? sx[g][c][p] - s00[g][c][p] - s11[g][c][p] : sx[g][c][p];
                    add128(acc, u128p{ cross << s, cross >> (64 - s) });
                    add128(acc, u128p{ s11[g][c][p] << (2 * s), s11[g][c][p] >> (64 - 2 * s) });
                    const u64 r = barrett128(acc, m);
                    if (KARA && !last) { s00[g][c][p] = r & lomask; sx[g][c][p] = (r & lomask) + (r >> s); }
                    else { s00[g][c][p] = r; sx[g][c][p] = 0; }
                    s11[g][c][p] = 0;
                }
    };

    const u32 cnt = job.cnt;
    Term A, B;                                                   // ping-pong register sets: no copies
    load_term(0, A);
    u32 in_chunk = 0;
    const u32 npairs = cnt >> 1;
    for (u32 pr = 0; pr < npairs; pr++) {                        // branch-free body: two terms per trip
        const u32 i = pr * 2;
        load_term(i + 1, B);
        mac_term(A);
        load_term(i + 2 < cnt ? i + 2 : cnt - 1, A);             // clamped prefetch (a re-read hits the cache)
        mac_term(B);
        in_chunk += 2;
        if (in_chunk + 3 > chunk) { fold(false); in_chunk = 1; } // the folded residue counts as one term
    }
    if (cnt & 1) mac_term(A);                                    // A holds the last term
    fold(true);
#pragma unroll
    for (int g = 0; g < G; g++) {
        if (g < (int)job.ng) {
            u64 *o = jp->out[g] + (size_t)b_limb * n + k;
            u64x2 r0, r1;
            r0[0] = s00[g][0][0]; r0[1] = s00[g][1][0];
            r1[0] = s00[g][0][1]; r1[1] = s00[g][1][1];
            *reinterpret_cast<u64x2 *>(o) = r0;
            *reinterpret_cast<u64x2 *>(o + job.out_poly_stride) = r1;
        }
    }
}

// ---- k_term_product, one lane: out[p][k] = a[k] * C_p[k] mod q_limb, p = 0, 1 (k_mac's fold of a single product IS barrett128 of it)
template <bool PACKED>
HD void term_product_lane(const DevLevel *__restrict__ lv, const TermJob *__restrict__ jobs, size_t njobs, size_t n, int limb, u32 pw_poly_stride,
                          u32 out_poly_stride, size_t k, size_t u)
{
    if (k >= n || u >= njobs) return;
    const TermJob job = jobs[u];
    const Mod m = lv->q[limb];
    u64 a0, a1;
    if constexpr (PACKED) {
        const u32 kb = lv->mac_bits[limb];
        u32 psh;
        const u32x4a4 w = ldg16_a4_nt(packed_window(job.pt, lv->mac_row_off[limb], k, kb, psh));
        packed_pair((u64)w[0] | ((u64)w[1] << 32), (u64)w[2] | ((u64)w[3] << 32), psh, kb, a0, a1);
    } else {
        const u64x2 a = ldg16_nt(job.pt + (size_t)limb * n + k);
        a0 = a[0]; a1 = a[1];
    }
    const u64 *pw = job.pw + (size_t)limb * n + k;
    const u64x2 c0 = ldg16(pw), c1 = ldg16(pw + pw_poly_stride);
    u64x2 r0, r1;
    r0[0] = barrett128(mul128(a0, c0[0]), m); r0[1] = barrett128(mul128(a1, c0[1]), m);
    r1[0] = barrett128(mul128(a0, c1[0]), m); r1[1] = barrett128(mul128(a1, c1[1]), m);
    *reinterpret_cast<u64x2 *>(job.out + k) = r0;
    *reinterpret_cast<u64x2 *>(job.out + out_poly_stride + k) = r1;
}

// ---- dense u64 limbs <-> rows of mac_bits[j] bits per coefficient, limb j of slot `slot`.  Pack, one lane per OUTPUT dword d: bits
// [32 d, 32 d + 32) of the row come from at most two coefficients (widths are >= 32); unpack, one lane per coefficient c
HD void pack_rows_lane(const DevLevel *__restrict__ lv, int L, const u64 *__restrict__ dense, char *__restrict__ packed, size_t slot_bytes, size_t n,
                       size_t d, size_t slot, int j)
{
    const u32 w = lv->mac_bits[j];
    const size_t ndw = n * w / 32;
    if (d >= ndw) return;
    const u64 *src = dense + (slot * L + j) * n;
    const size_t bit0 = d * 32, c0 = bit0 / w;
    const u32 off = (u32)(bit0 - c0 * w), got = w - off;
    u64 v = src[c0] >> off;
    if (got < 32 && c0 + 1 < n) v |= src[c0 + 1] << got;
    reinterpret_cast<u32 *>(packed + slot * slot_bytes + lv->mac_row_off[j])[d] = (u32)v;
}
HD void unpack_rows_lane(const DevLevel *__restrict__ lv, int L, const char *__restrict__ packed, size_t slot_bytes, u64 *__restrict__ dense, size_t n,
                         size_t c, size_t slot, int j)
{
    if (c >= n) return;
    const u32 w = lv->mac_bits[j];
    dense[(slot * L + j) * n + c] = packed_coeff(reinterpret_cast<const u32 *>(packed + slot * slot_bytes + lv->mac_row_off[j]), c, w);
}

} // namespace apsu_he
