// Hand-written gfx950 kernels of the homomorphic query-evaluation engine.
// Each kernel names the seal::Evaluator step it replaces and the reference call sites.
// Conventions: 64-lane waves, 256-thread workgroups for coefficient-parallel kernels (one thread
// per coefficient index, consecutive lanes on consecutive coefficients -> 512 B per wave access),
// level constants read through wave-uniform loads.  No MFMA: the work is modular-integer
// butterflies and dyadic products (BASELINE.json north_star).
#include "device.h"
#include "ntt_wg.h"
#include "bin_update.h"
#include "bin_lookup.h"
#include "bin_merge.h"
#include <cstdlib>
#include <type_traits>

#include <algorithm>

namespace apsu_he {

#define KERNEL_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) throw_hip(e_, __FILE__, __LINE__); } while (0)
void throw_hip(hipError_t e, const char *file, int line);

// ============================================================================ K1/K2: NTT
// transform_to_ntt_inplace / transform_from_ntt_inplace
// (receiver_osn.cpp:467,475 ; bin_bundle.cpp:154,268,297,321) and every NTT inside
// multiply / relinearize / multiply_plain.  One workgroup per limb polynomial, limb resident in LDS.
// (the workgroup body -- passes + synchronisation -- lives in ntt_wg.h)
// split != 0: the launch transforms the two HALVES of limbs twice this size (poly_modulus_degree 32768: one limb is 256 KiB and
// does not fit a workgroup's LDS).  Block g is half g & 1 of limb g >> 1 and takes table 2 * modulus + half, whose forward
// twiddles are the big transform's for that half (W_h[2^s + b] = W[2^(s+1) + h 2^s + b]); the first Cooley-Tukey stage runs in
// front (k_ntt_first_stage), the inverse's last stage and twist behind (k_ntt_last_stage), so the inverse halves are always RAW.
// C: coefficients per lane -- 16 (T = n / 16 threads per limb: the throughput form) or 8 (T = n / 8: the latency form of round 6 for
// launches that leave CUs idle, ntt_core.h plan_k; same bits).  MINW: waves per SIMD the register budget must admit (8: <= 64 VGPRs, two
// 1024-thread workgroups per CU at n = 8192).  Which form a launch takes: ntt_form (ntt_form.h).
template <int LOGN, bool INV, int T, int C = 16, int MINW = 4>
__global__ __launch_bounds__(T, MINW) void k_ntt(u64 *__restrict__ data, const NttTable *__restrict__ tabs,
                                           const int *__restrict__ modmap, int period, int split)
{
    constexpr int N = 1 << LOGN;
    __shared__ __attribute__((aligned(16))) u64 lds[lds_slots(N)];
    const int tid = threadIdx.x;
    const size_t g = blockIdx.x;
    const int mv = modmap[(split ? g >> 1 : g) % (size_t)period];
    const NttTable tab = tabs[split ? (((mv & NTT_MAP_MASK) << 1) | (int)(g & 1)) : (mv & NTT_MAP_MASK)];
    u64 *p = data + g * N;
    // (the inverse transform stages its limb into LDS with coalesced loads: SrcStaged, ntt_core.h)
    using SRC = std::conditional_t<INV, SrcStaged, SrcPlain>;
    if (INV && ((mv & NTT_MAP_RAW) || split)) {                                 // wave-uniform branches
        if (tab.narrow) ntt_body<LOGN, INV, NTT_NARROW, T, 0, INV, SRC, true, false, 0, -1, C>(lds, p, tab, tid, nullptr, SRC());
        else if (tab.wide_d4) ntt_body<LOGN, INV, NTT_WIDE_NEAR, T, 0, INV, SRC, true, false, 0, -1, C>(lds, p, tab, tid, nullptr, SRC());
        else ntt_body<LOGN, INV, NTT_WIDE, T, 0, INV, SRC, true, false, 0, -1, C>(lds, p, tab, tid, nullptr, SRC());
        return;
    }
    if (tab.narrow) ntt_body<LOGN, INV, NTT_NARROW, T, 0, false, SRC, true, false, 0, -1, C>(lds, p, tab, tid, nullptr, SRC());
    else if (tab.wide_d4) ntt_body<LOGN, INV, NTT_WIDE_NEAR, T, 0, false, SRC, true, false, 0, -1, C>(lds, p, tab, tid, nullptr, SRC());
    else ntt_body<LOGN, INV, NTT_WIDE, T, 0, false, SRC, true, false, 0, -1, C>(lds, p, tab, tid, nullptr, SRC());
}

// ---- poly_modulus_degree 32768: one radix-2 stage over global memory around two half-size LDS-resident transforms.
// Tables: entry 2 m (+ 1) of `tabs`; its ninv / ninv_q fields carry the first stage's twiddle psi^brv(1) (the twist comes
// from the scale table), dit and scale are the full-size tables.
// forward, first Cooley-Tukey stage: (x_j, x_{j + n/2}) -> (x + w y, x - w y), canonical; src != nullptr: limb g is gathered from
// src[g] (residues of another modulus, reduced on load: the key switch's decomposition)
__global__ __launch_bounds__(EW_T) void k_ntt_first_stage(const u64 *const *__restrict__ src, u64 *__restrict__ data, size_t n,
                                                          const NttTable *__restrict__ tabs, const int *__restrict__ modmap, int period)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x, h = n >> 1;
    if (k >= h) return;
    const size_t g = blockIdx.y;
    const NttTable tab = tabs[(modmap[g % (size_t)period] & NTT_MAP_MASK) << 1];
    const u64 *in = src ? src[g] : data + g * n;
    u64 x = in[k], y = in[k + h];
    if (src) { x = ntt_reduce_any(x, tab); y = ntt_reduce_any(y, tab); }
    const u64 v = mul_shoup(y, tab.ninv, tab.ninv_q, tab.q);
    u64 *out = data + g * n;
    out[k] = addmod(x, v, tab.q);
    out[k + h] = submod(x, v, tab.q);
}
// inverse, last decimation-in-time stage (E_j + w_j O_j, E_j - w_j O_j with w_j = psi^-2j) on the RAW outputs of the two
// half transforms, then the twist n^-1 psi^-j -- or, for a NTT_MAP_RAW limb, the raw sums for a consumer that applies it
__global__ __launch_bounds__(EW_T) void k_ntt_last_stage(u64 *__restrict__ data, size_t n, const NttTable *__restrict__ tabs,
                                                         const int *__restrict__ modmap, int period)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x, h = n >> 1;
    if (k >= h) return;
    const size_t g = blockIdx.y;
    const int mv = modmap[g % (size_t)period];
    const NttTable tab = tabs[(mv & NTT_MAP_MASK) << 1];
    u64 *p = data + g * n;
    const u64 q = tab.q;
    const u64x2 tw = ldg16(reinterpret_cast<const u64 *>(tab.dit + h + k));
    const u64 e = ntt_reduce_any(p[k], tab);                                    // [0, q)
    const u64 o = mul_shoup_lazy(p[k + h], tw[0], tw[1], q);                    // [0, 2q)
    u64 x0 = e + o, x1 = e + (q << 1) - o;                                      // < 3q, any consumer of RAW values takes them
    if (!(mv & NTT_MAP_RAW)) {
        const u64x2 s0 = ldg16(reinterpret_cast<const u64 *>(tab.scale + k)), s1 = ldg16(reinterpret_cast<const u64 *>(tab.scale + k + h));
        x0 = mul_shoup(x0, s0[0], s0[1], q);
        x1 = mul_shoup(x1, s1[0], s1[1], q);
    }
    p[k] = x0;
    p[k + h] = x1;
}

// Forward NTT of gathered limbs: limb g is read from src[g] (residues of another modulus, reduced on load) and written
// to data + g*N.  Replaces the decompose kernel of the key switch (App. B10): out[I][J] = NTT_I(c2_J mod m_I).
// C, MINW: as k_ntt (ntt_form picks them)
template <int LOGN, int T, int C = 16, int MINW = 4>
__global__ __launch_bounds__(T, MINW) void k_ntt_gather(const u64 *const *__restrict__ src, u64 *__restrict__ data,
                                                  const NttTable *__restrict__ tabs, const int *__restrict__ modmap, int period, int nored)
{
    constexpr int N = 1 << LOGN;
    __shared__ __attribute__((aligned(16))) u64 lds[lds_slots(N)];
    const int tid = threadIdx.x;
    const size_t g = blockIdx.x;
    const NttTable tab = tabs[modmap[g % (size_t)period]];
    u64 *p = data + g * N;
    // nored: every source residue fits the lazy range of every (narrow) target as it stands (checked by the host, ntt_gather_nored_ok):
    // the transform is linear and its closing reduction takes any 64-bit value, so the reduction on load is left out
    if (tab.narrow) {
        if (nored) ntt_body<LOGN, false, NTT_NARROW, T, 2, false, SrcPlain, true, false, 0, -1, C>(lds, p, tab, tid, src[g]);
        else ntt_body<LOGN, false, NTT_NARROW, T, 1, false, SrcPlain, true, false, 0, -1, C>(lds, p, tab, tid, src[g]);
    } else if (tab.wide_d4) ntt_body<LOGN, false, NTT_WIDE_NEAR, T, 1, false, SrcPlain, true, false, 0, -1, C>(lds, p, tab, tid, src[g]);
    else ntt_body<LOGN, false, NTT_WIDE, T, 1, false, SrcPlain, true, false, 0, -1, C>(lds, p, tab, tid, src[g]);
}

// Inverse NTT of dyadic tensor products (BEHZ steps 4 + 5 in one launch): workgroup g < n_tensor owns output limb
// (job, poly p of 3, limb e of `limbs`) of product job = g / (3*limbs), forms d_p = a0*b0 | a0*b1 + a1*b0 | a1*b1 in limb e from
// the NTT-form operands while it loads (SrcTensor) and writes the coefficient-form limb to job.d[p][e]: the tensor kernel,
// its 3*E limb writes and the transform's re-read of them are gone.  Workgroups g >= n_tensor transform
// plain[g - n_tensor] in place (limbs that join the same launch).  Operand polys are src_ps words apart.
template <int LOGN, int T, int C = 16>
__global__ __launch_bounds__(T, 4) void k_intt_tensor(const TensorJob *__restrict__ jobs, int limbs, size_t src_ps, size_t n_tensor,
                                                   u64 *__restrict__ plain, const NttTable *__restrict__ tabs,
                                                   const int *__restrict__ modmap, int period)
{
    constexpr int N = 1 << LOGN;
    __shared__ __attribute__((aligned(16))) u64 lds[lds_slots(N)];
    const int tid = threadIdx.x;
    size_t g = blockIdx.x;
    {
        // XCD-aware order: the three workgroups of one (product, limb) pair -- which read the same operand limbs -- sit 8 apart in
        // the grid (workgroups b and b + 8 share an XCD, hence an L2): pair u = 8 blk + lane, polynomial pl at 24 blk + 8 pl + lane.
        // (One product per block with lane = limb, so that all workgroups of limb e share an XCD and products with a common parent
        //  find it in that L2 too, measured level against this: profiles/r03_ab_xcd.txt.)
        const size_t pairs = n_tensor / 3, padded = (pairs + 7) / 8 * 24;
        if (g < padded) {
            const size_t blk = g / 24, rem = g - blk * 24, pl = rem >> 3, u = blk * 8 + (rem & 7);
            if (u >= pairs) return;                                             // wave-uniform: the padding of the last block of 8 pairs
            const size_t jb = u / (size_t)limbs, e = u - jb * limbs;
            g = jb * 3 * limbs + pl * limbs + e;                                // the logical index every table below is laid out by
        } else {
            g = n_tensor + (g - padded);
        }
    }
    const int mv = modmap[g % (size_t)period];
    const NttTable tab = tabs[mv & NTT_MAP_MASK];
    if (g >= n_tensor) {                                                        // wave-uniform
        u64 *p = plain + (g - n_tensor) * N;
        if (mv & NTT_MAP_RAW) {
            if (tab.narrow) ntt_body<LOGN, true, NTT_NARROW, T, 0, true, SrcStaged, true, false, 0, -1, C>(lds, p, tab, tid, nullptr, SrcStaged());
            else if (tab.wide_d4) ntt_body<LOGN, true, NTT_WIDE_NEAR, T, 0, true, SrcStaged, true, false, 0, -1, C>(lds, p, tab, tid, nullptr, SrcStaged());
            else ntt_body<LOGN, true, NTT_WIDE, T, 0, true, SrcStaged, true, false, 0, -1, C>(lds, p, tab, tid, nullptr, SrcStaged());
        } else {
            if (tab.narrow) ntt_body<LOGN, true, NTT_NARROW, T, 0, false, SrcStaged, true, false, 0, -1, C>(lds, p, tab, tid, nullptr, SrcStaged());
            else if (tab.wide_d4) ntt_body<LOGN, true, NTT_WIDE_NEAR, T, 0, false, SrcStaged, true, false, 0, -1, C>(lds, p, tab, tid, nullptr, SrcStaged());
            else ntt_body<LOGN, true, NTT_WIDE, T, 0, false, SrcStaged, true, false, 0, -1, C>(lds, p, tab, tid, nullptr, SrcStaged());
        }
        return;
    }
    const size_t per = (size_t)3 * limbs, jb = g / per;
    const int r = (int)(g - jb * per), pl = r / limbs, e = r - pl * limbs;
    const TensorJob job = jobs[jb];
    const u64 *a0 = job.a + (size_t)e * N, *a1 = a0 + src_ps, *b0 = job.b + (size_t)e * N, *b1 = b0 + src_ps;
    // the fold's last word (< 4q) enters the transform as it is where the range discipline takes that (-1.05 % query, profiles/r04_ab_tensor_lazy.txt)
    const bool lazy = ntt_lazy_input_ok(tab, LOGN);
    SrcTensor ops;
    if (pl == 0) ops = SrcTensor{ a0, b0, nullptr, nullptr, lazy };
    else if (pl == 1) ops = SrcTensor{ a0, b1, a1, b0, lazy };
    else ops = SrcTensor{ a1, b1, nullptr, nullptr, lazy };
    u64 *p = job.d + (size_t)r * N;
    if (mv & NTT_MAP_RAW) {
        if (tab.narrow) ntt_body<LOGN, true, NTT_NARROW, T, 0, true, SrcTensor, true, false, 0, -1, C>(lds, p, tab, tid, nullptr, ops);
        else if (tab.wide_d4) ntt_body<LOGN, true, NTT_WIDE_NEAR, T, 0, true, SrcTensor, true, false, 0, -1, C>(lds, p, tab, tid, nullptr, ops);
        else ntt_body<LOGN, true, NTT_WIDE, T, 0, true, SrcTensor, true, false, 0, -1, C>(lds, p, tab, tid, nullptr, ops);
    } else {
        if (tab.narrow) ntt_body<LOGN, true, NTT_NARROW, T, 0, false, SrcTensor, true, false, 0, -1, C>(lds, p, tab, tid, nullptr, ops);
        else if (tab.wide_d4) ntt_body<LOGN, true, NTT_WIDE_NEAR, T, 0, false, SrcTensor, true, false, 0, -1, C>(lds, p, tab, tid, nullptr, ops);
        else ntt_body<LOGN, true, NTT_WIDE, T, 0, false, SrcTensor, true, false, 0, -1, C>(lds, p, tab, tid, nullptr, ops);
    }
}

// ---- launch forms: ntt_form (ntt_form.h) picks the form, one instantiation table per kernel family holds the kernels it may pick
// (inverse / forward kernel of each form; the tables' order is the kernels' order in the code object)
template <class K> struct NttFormRow { int logn, threads, coeffs_per_lane, min_waves; K inv, fwd; };
template <class K, size_t R> static K form_kernel(const NttFormRow<K> (&rows)[R], int logn, const NttForm &f, bool inverse)
{
    for (const NttFormRow<K> &r : rows)
        if (r.logn == logn && r.threads == f.threads && r.coeffs_per_lane == f.coeffs_per_lane && r.min_waves == f.min_waves && (inverse ? r.inv : r.fwd))
            return inverse ? r.inv : r.fwd;
    throw_hip(hipErrorInvalidValue, __FILE__, __LINE__);
    return nullptr;
}

using GatherKernel = void (*)(const u64 *const *, u64 *, const NttTable *, const int *, int, int);
#define ROW(LN, T, C, W) { LN, T, C, W, nullptr, k_ntt_gather<LN, T, C, W> },
static const NttFormRow<GatherKernel> k_ntt_gather_forms[] = {
    ROW(13, 1024, 8, 4) ROW(12, 512, 8, 4) ROW(13, 1024, 8, 8)
    ROW(14, 1024, 16, 4) ROW(13, 512, 16, 4) ROW(12, 256, 16, 4) ROW(11, 128, 16, 4) ROW(10, 64, 16, 4) ROW(8, 64, 16, 4) ROW(6, 64, 16, 4)
};
#undef ROW
using TensorKernel = void (*)(const TensorJob *, int, size_t, size_t, u64 *, const NttTable *, const int *, int);
#define ROW(LN, T, C) { LN, T, C, 4, k_intt_tensor<LN, T, C>, nullptr },
static const NttFormRow<TensorKernel> k_intt_tensor_forms[] = {
    ROW(13, 1024, 8) ROW(12, 512, 8)
    ROW(14, 1024, 16) ROW(13, 512, 16) ROW(12, 256, 16) ROW(11, 128, 16) ROW(10, 64, 16) ROW(8, 64, 16) ROW(6, 64, 16)
};
#undef ROW
using NttKernel = void (*)(u64 *, const NttTable *, const int *, int, int);
#define ROW(LN, T, C, W) { LN, T, C, W, k_ntt<LN, true, T, C, W>, k_ntt<LN, false, T, C, W> },
static const NttFormRow<NttKernel> k_ntt_forms[] = {
    ROW(14, 1024, 16, 4)
    { 13, 1024, 8, 8, nullptr, k_ntt<13, false, 1024, 8, 8> },
    ROW(13, 1024, 8, 4) ROW(12, 512, 8, 4)
    ROW(13, 512, 16, 4) ROW(12, 256, 16, 4) ROW(11, 128, 16, 4) ROW(10, 64, 16, 4) ROW(8, 64, 16, 4) ROW(6, 64, 16, 4)
};
#undef ROW

// n = 32768 (f.split): the halves run in f's form at n = 16384; src != nullptr: the first stage gathers and reduces
static void launch_ntt_split(bool inverse, const u64 *const *src, u64 *data, size_t count, const NttTable *tabs, const int *modmap, int period,
                             hipStream_t st, const NttForm &f)
{
    const size_t n = (size_t)1 << SPLIT_LOGN;
    const dim3 g((unsigned)((n / 2 + EW_T - 1) / EW_T), (unsigned)count);
    if (!inverse) hipLaunchKernelGGL(k_ntt_first_stage, g, dim3(EW_T), 0, st, src, data, n, tabs, modmap, period);
    hipLaunchKernelGGL(form_kernel(k_ntt_forms, SPLIT_LOGN - 1, f, inverse), dim3((unsigned)(count * 2)), dim3(f.threads), 0, st,
                       data, tabs, modmap, period, 1);
    if (inverse) hipLaunchKernelGGL(k_ntt_last_stage, g, dim3(EW_T), 0, st, data, n, tabs, modmap, period);
}

void launch_ntt(int logn, bool inverse, u64 *data, size_t count, const NttTable *tabs, const int *modmap, int period,
                hipStream_t st, size_t latency_limbs, bool narrow)
{
    if (!count) return;
    const NttForm f = ntt_form(logn, inverse ? NTT_KIND_INVERSE : NTT_KIND_FORWARD, count, latency_limbs, narrow);
    if (f.split) launch_ntt_split(inverse, nullptr, data, count, tabs, modmap, period, st, f);
    else hipLaunchKernelGGL(form_kernel(k_ntt_forms, logn, f, inverse), dim3((unsigned)count), dim3(f.threads), 0, st, data, tabs, modmap, period, 0);
    KERNEL_CHECK();
}

void launch_ntt_gather(int logn, const u64 *const *src, u64 *data, size_t count, const NttTable *tabs, const int *modmap, int period,
                       hipStream_t st, bool nored, size_t latency_limbs, bool narrow)
{
    if (!count) return;
    const NttForm f = ntt_form(logn, NTT_KIND_GATHER, count, latency_limbs, narrow);
    if (f.split) launch_ntt_split(false, src, data, count, tabs, modmap, period, st, f);
    else hipLaunchKernelGGL(form_kernel(k_ntt_gather_forms, logn, f, false), dim3((unsigned)count), dim3(f.threads), 0, st, src, data, tabs, modmap, period, nored ? 1 : 0);
    KERNEL_CHECK();
}

void launch_intt_tensor(int logn, const TensorJob *jobs, int njobs, int limbs, size_t src_ps, u64 *plain, size_t n_plain,
                        const NttTable *tabs, const int *modmap, int period, hipStream_t st, size_t latency_limbs)
{
    const size_t n_tensor = (size_t)njobs * 3 * limbs;
    const size_t count = (n_tensor / 3 + 7) / 8 * 24 + n_plain;                 // the XCD-aware order pads the pairs to blocks of eight
    if (!(n_tensor + n_plain)) return;
    const NttForm f = ntt_form(logn, NTT_KIND_TENSOR, n_tensor + n_plain, latency_limbs, false);
    hipLaunchKernelGGL(form_kernel(k_intt_tensor_forms, logn, f, true), dim3((unsigned)count), dim3(f.threads), 0, st,
                       jobs, limbs, src_ps, n_tensor, plain, tabs, modmap, period);
    KERNEL_CHECK();
}

// ============================================================================ coefficient-parallel helpers
static inline dim3 ew_grid(size_t n, int batch) { return dim3((unsigned)((n + EW_T - 1) / EW_T), (unsigned)batch); }

// K3 (single term): multiply_plain on NTT ct x NTT plaintext (bin_bundle.cpp:147,258,287,320)
__global__ __launch_bounds__(EW_T) void k_dyadic_plain(const DevLevel *__restrict__ lv, const u64 *__restrict__ ct,
                                                       const u64 *__restrict__ pt, u64 *__restrict__ out, int polys,
                                                       size_t n, size_t pt_batch_stride)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const int L = lv->L;
    const size_t b = blockIdx.y;
    const u64 *a = ct + b * polys * L * n;
    const u64 *p = pt + b * pt_batch_stride;
    u64 *o = out + b * polys * L * n;
    for (int j = 0; j < L; j++) {
        const Mod m = lv->q[j];
        const u64 pv = p[j * n + k];
        for (int c = 0; c < polys; c++) o[(c * L + j) * n + k] = mulmod(a[(c * L + j) * n + k], pv, m);
    }
}

void launch_dyadic_plain(const DevLevel *lv, const u64 *ct, const u64 *pt, u64 *out, int polys, size_t n, int batch,
                         size_t pt_batch_stride, hipStream_t st)
{
    hipLaunchKernelGGL(k_dyadic_plain, ew_grid(n, batch), dim3(EW_T), 0, st, lv, ct, pt, out, polys, n, pt_batch_stride);
    KERNEL_CHECK();
}

// K10: add_inplace (bin_bundle.cpp:148,264,273,293,303,323,336)
__global__ __launch_bounds__(EW_T) void k_add(const DevLevel *__restrict__ lv, u64 *__restrict__ acc,
                                              const u64 *__restrict__ x, int polys, size_t n)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const int L = lv->L;
    const size_t off = (size_t)blockIdx.y * polys * L * n;
    for (int j = 0; j < L; j++) {
        const u64 q = lv->q[j].q;
        for (int c = 0; c < polys; c++) {
            const size_t i = off + (c * L + j) * n + k;
            acc[i] = addmod(acc[i], x[i], q);
        }
    }
}

void launch_add(const DevLevel *lv, u64 *acc, const u64 *x, int polys, size_t n, int batch, hipStream_t st)
{
    hipLaunchKernelGGL(k_add, ew_grid(n, batch), dim3(EW_T), 0, st, lv, acc, x, polys, n);
    KERNEL_CHECK();
}

// acc[b] += sum_i x[b][i]  — exact modular sum of `terms` ciphertexts (order-insensitive)
__global__ __launch_bounds__(EW_T) void k_add_many(const DevLevel *__restrict__ lv, u64 *__restrict__ acc, size_t acc_stride,
                                                   const u64 *__restrict__ x, int terms, int polys, size_t n)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const int L = lv->L;
    const size_t b = blockIdx.y;
    const size_t ctw = (size_t)polys * L * n;
    for (int j = 0; j < L; j++) {
        const u64 q = lv->q[j].q;
        for (int c = 0; c < polys; c++) {
            const size_t o = (c * L + j) * n + k;
            u64 s = acc[b * acc_stride + o];
            for (int i = 0; i < terms; i++) s = addmod(s, x[(b * terms + i) * ctw + o], q);
            acc[b * acc_stride + o] = s;
        }
    }
}

void launch_add_many(const DevLevel *lv, u64 *acc, size_t acc_stride, const u64 *x, int terms, int polys, size_t n,
                     int batch, hipStream_t st)
{
    hipLaunchKernelGGL(k_add_many, ew_grid(n, batch), dim3(EW_T), 0, st, lv, acc, acc_stride, x, terms, polys, n);
    KERNEL_CHECK();
}

// dst[polys][L][n] = sum over `terms` consecutive ciphertexts src[t][polys][L][n]  (exact modular sums)
__global__ __launch_bounds__(EW_T) void k_sum_jobs(const DevLevel *__restrict__ lv, const SumJob *__restrict__ jobs, int polys, size_t n)
{
    const size_t k = ((size_t)blockIdx.x * EW_T + threadIdx.x) * 2;
    if (k >= n) return;
    const int L = lv->L;
    const SumJob job = jobs[blockIdx.y / (polys * L)];
    const int pl = blockIdx.y % (polys * L);              // (poly, limb) pair
    const u64 q = lv->q[pl % L].q;
    const size_t ctw = (size_t)polys * L * n;
    const u64 *src = job.src + (size_t)pl * n + k;
    u64 s0 = 0, s1 = 0;
    for (int t = 0; t < job.terms; t++) {
        const u64x2 v = ldg16(src + (size_t)t * ctw);
        s0 = addmod(s0, v[0], q);
        s1 = addmod(s1, v[1], q);
    }
    u64x2 r; r[0] = s0; r[1] = s1;
    *reinterpret_cast<u64x2 *>(job.dst + (size_t)pl * n + k) = r;
}

void launch_sum_jobs(const DevLevel *lv, int L, const SumJob *jobs, int polys, size_t n, int njobs, hipStream_t st)
{
    if (!njobs) return;
    hipLaunchKernelGGL(k_sum_jobs, dim3((unsigned)((n / 2 + EW_T - 1) / EW_T), (unsigned)(njobs * polys * L)), dim3(EW_T), 0, st,
                       lv, jobs, polys, n);
    KERNEL_CHECK();
}

// Delta(m) of SEAL's BFV scaling (App. B7): round(m*Q/t) = m*floor(Q/t) + fix in RNS, fix = floor((m*(Q mod t) + floor((t+1)/2)) / t).
// Shared by add_plain and the querier's encryption (k_enc_finish).
__device__ __forceinline__ u64 plain_scale_fix(const DevLevel *__restrict__ lv, u64 m)
{
    // fix = floor((m * (Q mod t) + floor((t+1)/2)) / t), exact 128-by-64 division (m < t < 2^61)
    u128p num = mul128(m, lv->q_mod_t);
    add128(num, u128p{ lv->threshold, 0 });
    const u64 t = lv->t;
    u64 rem = num.hi % t, lo = num.lo, fix = 0;
    if (num.hi == 0) {
        fix = lo / t;
    } else {
        for (int i = 0; i < 64; i++) {                  // shift-subtract; only for t > 2^32
            rem = (rem << 1) | (lo >> 63);
            lo <<= 1;
            fix <<= 1;
            if (rem >= t) { rem -= t; fix |= 1; }
        }
    }
    return fix;
}
__device__ __forceinline__ u64 plain_scale_limb(const DevLevel *__restrict__ lv, int j, u64 m, u64 fix)
{
    u128p s = mul128(m, lv->coeff_div_plain[j]);
    add128(s, u128p{ fix, 0 });
    return barrett128(s, lv->q[j]);
}

// K8: add_plain_inplace (bin_bundle.cpp:159,162,345,346): c0 += round(m*Q/t) in RNS  (App. B7)
__global__ __launch_bounds__(EW_T) void k_add_plain(const DevLevel *__restrict__ lv, const PlainJob *__restrict__ jobs, size_t n)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const PlainJob job = jobs[blockIdx.y];
    const u64 m = job.pt[k];
    const u64 fix = plain_scale_fix(lv, m);
    u64 *c0 = job.ct;
    for (int j = 0; j < lv->L; j++) {
        const u64 scaled = plain_scale_limb(lv, j, m, fix);
        c0[j * n + k] = addmod(c0[j * n + k], scaled, lv->q[j].q);
    }
}

void launch_add_plain(const DevLevel *lv, const PlainJob *jobs, size_t n, int batch, hipStream_t st)
{
    if (!batch) return;
    hipLaunchKernelGGL(k_add_plain, ew_grid(n, batch), dim3(EW_T), 0, st, lv, jobs, n);
    KERNEL_CHECK();
}

// K4 (first half): plaintext lift mod t -> RNS (App. B5); NTT follows as a separate launch.
// no_lift[b] != 0 selects SEAL's monomial shortcut (value copied unlifted).
__global__ __launch_bounds__(EW_T) void k_lift(const DevLevel *__restrict__ lv, const u64 *__restrict__ pt,
                                               u64 *__restrict__ out, size_t n, const unsigned char *__restrict__ no_lift)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const size_t b = blockIdx.y;
    const u64 v = pt[b * n + k];
    const bool lift = (v >= lv->threshold) && !(no_lift && no_lift[b]);
    const int L = lv->L;
    for (int j = 0; j < L; j++) out[(b * L + j) * n + k] = lift ? v + lv->incr[j] : v;
}

void launch_lift(const DevLevel *lv, const u64 *pt, u64 *out, size_t n, int batch, const unsigned char *no_lift,
                 hipStream_t st)
{
    hipLaunchKernelGGL(k_lift, ew_grid(n, batch), dim3(EW_T), 0, st, lv, pt, out, n, no_lift);
    KERNEL_CHECK();
}

// K7: mod_switch_to_next_inplace / mod_switch_to_inplace
// (receiver_osn.cpp:463,471,478 ; bin_bundle.cpp:169,269,298,322,335,355): drop q_last with rounding (B8)
// in: ciphertext c at in + c*in_stride holds `polys` polynomials [L][n]; out: packed [c][polys][L-1][n]
__global__ __launch_bounds__(EW_T) void k_modswitch(const DevLevel *__restrict__ lv, const u64 *__restrict__ in,
                                                    size_t in_stride, int polys, u64 *__restrict__ out, size_t n)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const int L = lv->L;
    const size_t c = blockIdx.y / polys, p = blockIdx.y % polys;
    const u64 *src = in + c * in_stride + p * (size_t)L * n;
    u64 *dst = out + (size_t)blockIdx.y * (L - 1) * n;
    const u64 ql = lv->q[L - 1].q;
    const u64 last = addmod(src[(size_t)(L - 1) * n + k], lv->half, ql);
    for (int j = 0; j + 1 < L; j++) {
        const Mod m = lv->q[j];
        const u64 tmp = submod(barrett64(last, m), lv->half_mod[j], m.q);
        const u64 v = submod(src[(size_t)j * n + k], tmp, m.q);
        dst[(size_t)j * n + k] = mul_shoup(v, lv->inv_q_last[j].w, lv->inv_q_last[j].wq, m.q);
    }
}

void launch_modswitch(const DevLevel *lv, const u64 *in, size_t in_stride, int polys, u64 *out, size_t n, int cts,
                      hipStream_t st)
{
    if (!cts) return;
    hipLaunchKernelGGL(k_modswitch, ew_grid(n, cts * polys), dim3(EW_T), 0, st, lv, in, in_stride, polys, out, n);
    KERNEL_CHECK();
}

// job-addressed variant used when the source ciphertexts are scattered (PowersDag slot order)
__global__ __launch_bounds__(EW_T) void k_modswitch_jobs(const DevLevel *__restrict__ lv, const CtJob *__restrict__ jobs,
                                                         int polys, size_t n)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const int L = lv->L;
    const CtJob job = jobs[blockIdx.y / polys];
    const size_t p = blockIdx.y % polys;
    const u64 *src = job.src + p * (size_t)L * n;
    u64 *dst = job.dst + p * (size_t)(L - 1) * n;
    const u64 ql = lv->q[L - 1].q;
    const u64 last = addmod(src[(size_t)(L - 1) * n + k], lv->half, ql);
    for (int j = 0; j + 1 < L; j++) {
        const Mod m = lv->q[j];
        const u64 tmp = submod(barrett64(last, m), lv->half_mod[j], m.q);
        const u64 v = submod(src[(size_t)j * n + k], tmp, m.q);
        dst[(size_t)j * n + k] = mul_shoup(v, lv->inv_q_last[j].w, lv->inv_q_last[j].wq, m.q);
    }
}

void launch_modswitch_jobs(const DevLevel *lv, const CtJob *jobs, int polys, size_t n, int njobs, hipStream_t st)
{
    if (!njobs) return;
    hipLaunchKernelGGL(k_modswitch_jobs, ew_grid(n, njobs * polys), dim3(EW_T), 0, st, lv, jobs, polys, n);
    KERNEL_CHECK();
}

__global__ __launch_bounds__(EW_T) void k_copy_jobs(const CtJob *__restrict__ jobs, size_t words)
{
    const CtJob job = jobs[blockIdx.y];
    for (size_t k = ((size_t)blockIdx.x * EW_T + threadIdx.x) * 2; k < words; k += (size_t)gridDim.x * EW_T * 2)
        *reinterpret_cast<u64x2 *>(job.dst + k) = *reinterpret_cast<const u64x2 *>(job.src + k);
}

// The same for the source ciphertexts of a query ([2][L][n] each): while it copies, every word is held against the prime of its limb
// (seal::is_data_valid_for); a word outside [0, q) writes the query's sequence number `seq` to *bad -- a word of page-locked host memory
// the engine looks at when it next waits for the device (one word per query in flight, so the report names the query: round 6).  The lazy
// transforms take source limbs as they are, so such a word must not pass silently.  src == dst: a check in place (sources that came from
// the host by a plain copy).
__global__ __launch_bounds__(EW_T) void k_copy_sources(const CtJob *__restrict__ jobs, size_t words, const DevLevel *__restrict__ lv, int L, size_t n,
                                                       unsigned *__restrict__ bad, unsigned seq)
{
    const CtJob job = jobs[blockIdx.y];
    bool wrong = false;
    for (size_t k = ((size_t)blockIdx.x * EW_T + threadIdx.x) * 2; k < words; k += (size_t)gridDim.x * EW_T * 2) {
        const u64x2 v = *reinterpret_cast<const u64x2 *>(job.src + k);
        const u64 q = lv->q[(k / n) % (size_t)L].q;                 // (n is even: both words lie in the same limb)
        wrong |= v[0] >= q || v[1] >= q;
        if (job.dst != job.src) *reinterpret_cast<u64x2 *>(job.dst + k) = v;
    }
    if (wrong) atomicMax(bad, seq);
}

void launch_copy_sources(const CtJob *jobs, size_t words, int njobs, const DevLevel *lv, int L, size_t n, unsigned *bad, unsigned seq, hipStream_t st)
{
    if (!njobs) return;
    unsigned gx = (unsigned)std::min<size_t>((words / 2 + EW_T - 1) / EW_T, 64);
    hipLaunchKernelGGL(k_copy_sources, dim3(gx, (unsigned)njobs), dim3(EW_T), 0, st, jobs, words, lv, L, n, bad, seq);
    KERNEL_CHECK();
}

void launch_copy_jobs(const CtJob *jobs, size_t words, int njobs, hipStream_t st)
{
    if (!njobs) return;
    unsigned gx = (unsigned)std::min<size_t>((words / 2 + EW_T - 1) / EW_T, 64);
    hipLaunchKernelGGL(k_copy_jobs, dim3(gx, (unsigned)njobs), dim3(EW_T), 0, st, jobs, words);
    KERNEL_CHECK();
}

// counter-based generator for synthetic DB plaintexts: out[i] = splitmix64(seed + i) % bound
// (documented so tests can regenerate the same values on the host)
__global__ __launch_bounds__(EW_T) void k_fill_random(u64 *__restrict__ out, size_t words, u64 seed, u64 bound)
{
    const size_t i = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (i >= words) return;
    u64 z = seed + (u64)i * 0x9e3779b97f4a7c15ULL + 0x9e3779b97f4a7c15ULL;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    z ^= z >> 31;
    out[i] = z % bound;
}

void launch_fill_random(u64 *out, size_t words, u64 seed, u64 bound, hipStream_t st)
{
    if (!words) return;
    hipLaunchKernelGGL(k_fill_random, dim3((unsigned)((words + EW_T - 1) / EW_T)), dim3(EW_T), 0, st, out, words, seed, bound);
    KERNEL_CHECK();
}

// Mask values as the reference draws them (receiver_osn.cpp:221-224,248-251): SEAL's Blake2xb generator under a 64-byte seed,
// out[i] = generate() % bound with the 32-bit generate(), i = the (first + i)-th output of the generator.  One lane per
// 64-byte stream block (16 values): it derives the root hash of its 4096-byte buffer and its own expansion node (3 BLAKE2b
// compressions; the redundant root hashes are ~2 us of work for a whole query's masks).
__global__ __launch_bounds__(EW_T) void k_fill_blake2xb(u64 *__restrict__ out, size_t words, Blake2xbSeed seed, u64 first, u64 bound)
{
    const u64 sb = first / 16 + (u64)blockIdx.x * EW_T + threadIdx.x;       // stream block of this lane
    if (sb * 16 >= first + words) return;
    u64 blk[8];
    blake2xb_stream_block(seed, sb, blk);
#pragma unroll
    for (unsigned j = 0; j < 16; j++) {
        const u64 g = sb * 16 + j;
        if (g >= first && g < first + words) out[g - first] = (u64)blake2xb_stream_u32(blk, j) % bound;
    }
}

void launch_fill_blake2xb(u64 *out, size_t words, const Blake2xbSeed &seed, u64 first, u64 bound, hipStream_t st)
{
    if (!words) return;
    const u64 blocks = (first + words + 15) / 16 - first / 16;
    hipLaunchKernelGGL(k_fill_blake2xb, dim3((unsigned)((blocks + EW_T - 1) / EW_T)), dim3(EW_T), 0, st, out, words, seed, first, bound);
    KERNEL_CHECK();
}

// N3 on the device: util::sample_poly_uniform under SEAL's Blake2xb generator (seal_codec.h) -- the c1 of a seeded ciphertext
// (Encryptor::encrypt_symmetric -> Serializable<Ciphertext>, sender/apsu/plaintext_powers.cpp:41-46) or of a seeded key.
// Pass 1 (k_seed_bulk): one lane per 64-byte stream block fills dst[L][n] with the generator's first L*n words reduced mod
// q_j; a word at or above the largest multiple of q_j below 2^64 - 1 is rejected and its position appended to the job's list.
// Pass 2 (k_seed_fix, one wave per ciphertext): the rejected positions are put in stream order (rank sort in LDS) and
// replaced one after the other by fresh draws that continue behind the bulk fill, exactly in SEAL's order; the wave
// generates 64 stream blocks at a time, every lane follows the same (uniform) control flow and lane 0 writes.
constexpr u32 SEED_REJ_CAP = 8192;                                // rejected positions per ciphertext the fix-up can hold
__global__ __launch_bounds__(EW_T) void k_seed_bulk(const SeedJob *__restrict__ jobs, const DevLevel *__restrict__ lv, const u64 *__restrict__ max_multiple,
                                                    size_t n, u32 *__restrict__ rej)
{
    const u64 sb = (u64)blockIdx.x * EW_T + threadIdx.x;
    const int L = lv->L;
    if (sb * 8 >= (u64)L * n) return;
    const SeedJob job = jobs[blockIdx.y];
    u64 blk[8];
    blake2xb_stream_block(job.seed, sb, blk);
    u32 *list = rej + (size_t)blockIdx.y * (1 + SEED_REJ_CAP);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const u64 w = sb * 8 + i;                                 // n is a multiple of 8: the block lies inside one limb
        const int j = (int)(w / n);
        if (blk[i] >= max_multiple[j]) {
            const u32 slot = atomicAdd(list, 1u);
            if (slot < SEED_REJ_CAP) list[1 + slot] = (u32)w;
        } else job.dst[w] = barrett64(blk[i], lv->q[j]);
    }
}

__global__ __launch_bounds__(64) void k_seed_fix(const SeedJob *__restrict__ jobs, const DevLevel *__restrict__ lv, const u64 *__restrict__ max_multiple,
                                                 size_t n, u32 *__restrict__ rej, int *__restrict__ overflow)
{
    __shared__ u32 sorted[SEED_REJ_CAP];
    __shared__ u64 cache[64 * 8];
    const SeedJob job = jobs[blockIdx.x];
    u32 *list = rej + (size_t)blockIdx.x * (1 + SEED_REJ_CAP);
    const u32 cnt = list[0];
    const u32 lane = threadIdx.x;
    if (cnt > SEED_REJ_CAP) { if (lane == 0) *overflow = 1; return; }
    for (u32 e = lane; e < cnt; e += 64) {                        // rank sort (positions are distinct)
        const u32 v = list[1 + e];
        u32 rank = 0;
        for (u32 k = 0; k < cnt; k++) rank += list[1 + k] < v;
        sorted[rank] = v;
    }
    __syncthreads();
    u64 next = (u64)lv->L * n;                                    // fresh draws continue behind the bulk fill
    u64 cache_block = ~(u64)0;                                    // first stream block held in `cache`
    for (u32 k = 0; k < cnt; k++) {                               // uniform: every lane walks the same list
        const u32 w = sorted[k];
        const int j = (int)(w / n);
        const u64 mm = max_multiple[j];
        u64 r;
        do {
            const u64 b = next >> 3;
            if (cache_block == ~(u64)0 || b < cache_block || b >= cache_block + 64) {
                __syncthreads();
                cache_block = b;
                u64 blk[8];
                blake2xb_stream_block(job.seed, b + lane, blk);
#pragma unroll
                for (int i = 0; i < 8; i++) cache[lane * 8 + i] = blk[i];
                __syncthreads();
            }
            r = cache[(next - (cache_block << 3))];
            next++;
        } while (r >= mm);
        if (lane == 0) job.dst[w] = barrett64(r, lv->q[j]);
    }
    if (lane == 0) list[0] = 0;                                   // ready for the next use of this list
}

void launch_seed_expand(const SeedJob *jobs, int njobs, const DevLevel *lv, int L, const u64 *max_multiple, size_t n, u32 *rej, int *overflow,
                        hipStream_t st)
{
    if (!njobs) return;
    const u64 blocks = ((u64)L * n + 7) / 8;
    hipLaunchKernelGGL(k_seed_bulk, dim3((unsigned)((blocks + EW_T - 1) / EW_T), (unsigned)njobs), dim3(EW_T), 0, st, jobs, lv, max_multiple, n, rej);
    hipLaunchKernelGGL(k_seed_fix, dim3((unsigned)njobs), dim3(64), 0, st, jobs, lv, max_multiple, n, rej, overflow);
    KERNEL_CHECK();
}

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

// N4: the querier's decryption of a result at the last level (result_package.cpp:175-213, Decryptor::decrypt):
// x = c0 + v (v = INTT(NTT(c1) . s), one limb q0), m = round(t x / q0) mod t.
// rem receives (t x + floor(q0 / 2)) mod q0
__device__ __forceinline__ u64 decrypt_round_coeff(u64 x, u64 q0, u64 t, u64 &rem)
{
    u128p num = mul128(x, t);
    add128(num, u128p{ q0 >> 1, 0 });
    // floor(num / q0) mod t by restoring division, the quotient folded mod t on the fly (num < 2^124)
    u64 quo = 0;
    rem = 0;
    for (int i = 127; i >= 0; i--) {
        const u64 bit = i >= 64 ? (num.hi >> (i - 64)) & 1 : (num.lo >> i) & 1;
        rem = (rem << 1) | bit;                                   // rem < q0 < 2^62 before the shift
        quo <<= 1;                                                // quo < t < 2^61
        if (rem >= q0) { rem -= q0; quo |= 1; }
        if (quo >= t) quo -= t;
    }
    return quo;
}

__global__ __launch_bounds__(EW_T) void k_decrypt_round(const u64 *__restrict__ ct, size_t ct_stride, const u64 *__restrict__ v,
                                                        u64 q0, u64 t, u64 *__restrict__ out, size_t n)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const size_t b = blockIdx.y;
    const u64 x = addmod(ct[b * ct_stride + k], v[b * n + k], q0);
    u64 rem;
    out[b * n + k] = decrypt_round_coeff(x, q0, t, rem);
}

// The same with SEAL's invariant noise budget (result_package.cpp:175-213, Decryptor::invariant_noise_budget): worst[b] = the
// largest centred |t x mod q0| over ciphertext b's coefficients; budget = floor(log2(q0 / (2 worst))) is formed on the host.
// Wave maximum, then the workgroup's four waves through LDS and one atomic per workgroup.
__global__ __launch_bounds__(EW_T) void k_decrypt_round_budget(const u64 *__restrict__ ct, size_t ct_stride, const u64 *__restrict__ v,
                                                               u64 q0, u64 t, u64 *__restrict__ out, size_t n, unsigned long long *__restrict__ worst)
{
    __shared__ u64 wave_max[EW_T / 64];
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    const size_t b = blockIdx.y;
    u64 dist = 0;
    if (k < n) {
        const u64 x = addmod(ct[b * ct_stride + k], v[b * n + k], q0);
        u64 rem;
        out[b * n + k] = decrypt_round_coeff(x, q0, t, rem);
        const u64 r = submod(rem, q0 >> 1, q0);                   // t x mod q0
        dist = r > (q0 >> 1) ? q0 - r : r;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const u64 o = (u64)__shfl_xor((unsigned long long)dist, off, 64);
        dist = o > dist ? o : dist;
    }
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = dist;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < EW_T / 64; w++) dist = wave_max[w] > dist ? wave_max[w] : dist;
        atomicMax(worst + b, (unsigned long long)dist);
    }
}

void launch_decrypt_round(const u64 *ct, size_t ct_stride, const u64 *v, u64 q0, u64 t, u64 *out, size_t n, int batch, hipStream_t st)
{
    if (!batch) return;
    hipLaunchKernelGGL(k_decrypt_round, ew_grid(n, batch), dim3(EW_T), 0, st, ct, ct_stride, v, q0, t, out, n);
    KERNEL_CHECK();
}

void launch_decrypt_round_budget(const u64 *ct, size_t ct_stride, const u64 *v, u64 q0, u64 t, u64 *out, size_t n, int batch, u64 *worst,
                                 hipStream_t st)
{
    if (!batch) return;
    hipLaunchKernelGGL(k_decrypt_round_budget, ew_grid(n, batch), dim3(EW_T), 0, st, ct, ct_stride, v, q0, t, out, n,
                       reinterpret_cast<unsigned long long *>(worst));
    KERNEL_CHECK();
}

// ============================================================================ N5: the querier's side (query_side.h)
// PlaintextPowers (sender/apsu/plaintext_powers.cpp:51-99) + the slot permutation of BatchEncoder::encode: for bundle index b
// (blockIdx.y) and slot i, out[b * S + s][slot_map[i]] = x[b][i]^exps[s] mod t; the inverse NTT mod t follows.  The exponent bits
// are wave-uniform.  A value >= t raises QS_FLAG_VALUE (and counts as 0).
__global__ __launch_bounds__(EW_T) void k_plain_powers(const u64 *__restrict__ vals, const u32 *__restrict__ slot_map, const u32 *__restrict__ exps,
                                                       int S, Mod t, u64 *__restrict__ out, size_t n, u32 *__restrict__ flags)
{
    const size_t i = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (i >= n) return;
    const size_t b = blockIdx.y;
    u64 x = vals[b * n + i];
    if (x >= t.q) { atomicOr(flags, QS_FLAG_VALUE); x = 0; }
    const u32 dst = slot_map[i];
    for (int s = 0; s < S; s++) out[(b * S + s) * n + dst] = qs_pow_mod(x, exps[s], t);
}

void launch_plain_powers(const u64 *vals, const u32 *slot_map, const u32 *exps, int S, Mod t, u64 *out, size_t n, int batch, u32 *flags, hipStream_t st)
{
    if (!batch || !S) return;
    hipLaunchKernelGGL(k_plain_powers, ew_grid(n, batch), dim3(EW_T), 0, st, vals, slot_map, exps, S, t, out, n, flags);
    KERNEL_CHECK();
}

// The two samplers: one lane per 64-byte stream block (as k_fill_blake2xb) = eight coefficients, written once as eight signed
// bytes; the residues modulo each prime are formed by the consumers.  out: [n] resp. [count][n] int8, n a multiple of 8.
__global__ __launch_bounds__(EW_T) void k_sample_ternary(Blake2xbSeed seed, u64 *__restrict__ out, size_t n)
{
    const size_t g = (size_t)blockIdx.x * EW_T + threadIdx.x;     // group of eight coefficients
    if (g * 8 >= n) return;
    u64 blk[8], packed = 0;
    blake2xb_stream_block(seed, qs_secret_block(g * 8), blk);
#pragma unroll
    for (int i = 0; i < 8; i++) packed |= (u64)(unsigned char)(signed char)qs_ternary(blk[i]) << (8 * i);
    out[g] = packed;
}

__global__ __launch_bounds__(EW_T) void k_sample_cbd(Blake2xbSeed seed, u64 first_object, u64 *__restrict__ out, size_t n)
{
    const size_t g = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (g * 8 >= n) return;
    const size_t c = blockIdx.y;
    u64 blk[8], packed = 0;
    blake2xb_stream_block(seed, qs_noise_block(first_object + c, g * 8), blk);
#pragma unroll
    for (int i = 0; i < 8; i++) packed |= (u64)(unsigned char)(signed char)qs_cbd(blk[i]) << (8 * i);
    out[c * (n / 8) + g] = packed;
}

void launch_sample_ternary(const Blake2xbSeed &seed, signed char *out, size_t n, hipStream_t st)
{
    hipLaunchKernelGGL(k_sample_ternary, dim3((unsigned)((n / 8 + EW_T - 1) / EW_T)), dim3(EW_T), 0, st, seed, reinterpret_cast<u64 *>(out), n);
    KERNEL_CHECK();
}

void launch_sample_cbd(const Blake2xbSeed &seed, u64 first_object, signed char *out, size_t n, int count, hipStream_t st)
{
    if (!count) return;
    hipLaunchKernelGGL(k_sample_cbd, ew_grid(n / 8, count), dim3(EW_T), 0, st, seed, first_object, reinterpret_cast<u64 *>(out), n);
    KERNEL_CHECK();
}

// small signed polynomials as residues of the key primes: dst[c][j][k] = small[c][k] mod q_j, j < limbs  (blockIdx.y = c * limbs + j)
__global__ __launch_bounds__(EW_T) void k_small_lift(const DevKey *__restrict__ key, const signed char *__restrict__ small, u64 *__restrict__ dst,
                                                     int limbs, size_t n)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const size_t c = blockIdx.y / limbs;
    const int j = (int)(blockIdx.y % limbs);
    dst[(size_t)blockIdx.y * n + k] = qs_residue(small[c * n + k], key->q[j].q);
}

void launch_small_lift(const DevKey *key, const signed char *small, u64 *dst, int limbs, size_t n, int count, hipStream_t st)
{
    if (!count) return;
    hipLaunchKernelGGL(k_small_lift, ew_grid(n, count * limbs), dim3(EW_T), 0, st, key, small, dst, limbs, n);
    KERNEL_CHECK();
}

// Encryptor::encrypt_symmetric's closing step for ciphertext c = blockIdx.y, one lane per coefficient across the limbs:
// c0_j = Delta(m)_j - e - (c1 s)_j, canonical.  cts: [count][2][L][n] (c1 already in place), v: [count][L][n] = c1 s in coefficient
// form, pt: [count][n] mod t, e: [count][n] int8.
__global__ __launch_bounds__(EW_T) void k_enc_finish(const DevLevel *__restrict__ lv, const u64 *__restrict__ pt, const u64 *__restrict__ v,
                                                     const signed char *__restrict__ e, u64 *__restrict__ cts, size_t n)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const size_t c = blockIdx.y;
    const int L = lv->L;
    const u64 m = pt[c * n + k];
    const u64 fix = plain_scale_fix(lv, m);
    const int ek = e[c * n + k];
    const u64 *vc = v + c * L * n;
    u64 *c0 = cts + c * 2 * L * n;
    for (int j = 0; j < L; j++) {
        const u64 q = lv->q[j].q;
        const u64 x = submod(plain_scale_limb(lv, j, m, fix), qs_residue(ek, q), q);
        c0[j * n + k] = submod(x, vc[j * n + k], q);
    }
}

void launch_enc_finish(const DevLevel *lv, const u64 *pt, const u64 *v, const signed char *e, u64 *cts, size_t n, int count, hipStream_t st)
{
    if (!count) return;
    hipLaunchKernelGGL(k_enc_finish, ew_grid(n, count), dim3(EW_T), 0, st, lv, pt, v, e, cts, n);
    KERNEL_CHECK();
}

// KeyGenerator::create_relin_keys' closing step in the NTT domain, key i and limb j = blockIdx.y / K, % K:
// ksk[i][0][j] = -(a s + e) + [j == i] (p mod q_i) s^2, a = ksk[i][1][j], e: [K-1][K][n] (NTT form), s: [K][n], p = the special prime
__global__ __launch_bounds__(EW_T) void k_rlk_finish(const DevKey *__restrict__ key, const u64 *__restrict__ s, const u64 *__restrict__ e,
                                                     u64 *__restrict__ ksk, size_t n)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const int K = key->K;
    const int i = (int)(blockIdx.y / K), j = (int)(blockIdx.y % K);
    const Mod mq = key->q[j];
    const u64 sk = s[(size_t)j * n + k];
    u64 *c0 = ksk + ((size_t)i * 2 * K + j) * n, *a = c0 + (size_t)K * n;
    u64 r = submod(0, addmod(mulmod(a[k], sk, mq), e[((size_t)i * K + j) * n + k], mq.q), mq.q);
    if (j == i) r = addmod(r, mulmod(mulmod(sk, sk, mq), barrett64(key->q[K - 1].q, mq), mq), mq.q);
    c0[k] = r;
}

void launch_rlk_finish(const DevKey *key, int K, const u64 *s, const u64 *e, u64 *ksk, size_t n, hipStream_t st)
{
    if (K < 2) return;
    hipLaunchKernelGGL(k_rlk_finish, ew_grid(n, (K - 1) * K), dim3(EW_T), 0, st, key, s, e, ksk, n);
    KERNEL_CHECK();
}

// flag[b] = 1 iff plaintext b has exactly one non-zero coefficient (SEAL's monomial shortcut in multiply_plain)
__global__ __launch_bounds__(EW_T) void k_flag_monomial(const u64 *__restrict__ pt, size_t n, unsigned char *__restrict__ flag)
{
    __shared__ unsigned int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    unsigned int local = 0;
    for (size_t k = threadIdx.x; k < n; k += EW_T) local += pt[(size_t)blockIdx.x * n + k] != 0;
    atomicAdd(&cnt, local);
    __syncthreads();
    if (threadIdx.x == 0) flag[blockIdx.x] = cnt == 1 ? 1 : 0;
}

void launch_flag_monomial(const u64 *pt, size_t n, int batch, unsigned char *flag, hipStream_t st)
{
    if (!batch) return;
    hipLaunchKernelGGL(k_flag_monomial, dim3((unsigned)batch), dim3(EW_T), 0, st, pt, n, flag);
    KERNEL_CHECK();
}

// K9: try_clear_irrelevant_bits (bin_bundle.cpp:67-97)
__global__ __launch_bounds__(EW_T) void k_clear_bits(u64 *__restrict__ ct, size_t words, u64 mask)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k < words) ct[k] &= mask;
}

void launch_clear_bits(u64 *ct, size_t words, int bits, hipStream_t st)
{
    if (bits <= 0) return;
    hipLaunchKernelGGL(k_clear_bits, dim3((unsigned)((words + EW_T - 1) / EW_T)), dim3(EW_T), 0, st, ct, words,
                       ~(((u64)1 << bits) - 1));
    KERNEL_CHECK();
}

// ============================================================================ K5: BFV multiply (BEHZ)
// square / multiply / multiply_inplace (receiver_osn.cpp:422,424 ; bin_bundle.cpp:272,301)
//
// Step (1)+(2): q -> q u Bsk with Montgomery removal of the q-overflow (fastbconv_m_tilde + sm_mrq).
// in: [batch] polynomials [L][n] at stride in_stride ; out: [batch][E][n] (q part copied, Bsk part computed)
// TL / TNB > 0: compile-time limb counts (loops fully unrolled, constants fetched in bulk); 0 = generic.
template <int TL, int TNB>
__global__ __launch_bounds__(EW_T) void k_behz_ext(const DevLevel *__restrict__ lv, const u64 *__restrict__ in,
                                                   size_t in_stride, int polys, u64 *__restrict__ out, size_t n)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const int L = TL ? TL : lv->L, nBsk = TL ? TNB + 1 : lv->nBsk, E = L + nBsk;
    constexpr int LMAX = TL ? TL : DMAXL;
    constexpr int BMAX = TL ? TNB + 1 : DMAXB;
    const size_t c = blockIdx.y / polys, p = blockIdx.y % polys;
    const u64 *src = in + c * in_stride + p * (size_t)L * n;
    u64 *dst = out + (size_t)blockIdx.y * E * n;
    u64 xs[LMAX];
    u32 mt_acc = 0;
#pragma unroll
    for (int j = 0; j < LMAX; j++) {
        if (TL || j < L) {
            const u64 x = src[(size_t)j * n + k];
            dst[(size_t)j * n + k] = x;
            xs[j] = mul_shoup(x, lv->ext_scale[j].w, lv->ext_scale[j].wq, lv->q[j].q);
            mt_acc += (u32)xs[j] * lv->q_to_mt[j];           // arithmetic mod 2^32 = m_tilde
        }
    }
    const u32 r32 = mt_acc * lv->neg_inv_q_mt;
#pragma unroll
    for (int i = 0; i < BMAX; i++) {
        if (TL || i < nBsk) {
            const Mod m = lv->bsk[i];
            u128p acc{ 0, 0 };
#pragma unroll
            for (int j = 0; j < LMAX; j++)
                if (TL || j < L) mac128(acc, xs[j], lv->q_to_bsk[i][j]);
            const u64 y = barrett128(acc, m);
            // centred lift of r into Z_m (m_tilde is a power of two: ">=")
            u64 r = r32;
            if (r32 >= 0x80000000u) r += m.q - ((u64)1 << 32);
            u128p v = mul128(r, lv->prod_q_bsk[i]);
            add128(v, u128p{ y, 0 });
            const u64 red = barrett128(v, m);
            dst[(size_t)(L + i) * n + k] = mul_shoup(red, lv->inv_mt_bsk[i].w, lv->inv_mt_bsk[i].wq, m.q);
        }
    }
}

HD u64 lazy2(u64 x, const ShoupConst &c, u64 q) { return mul_shoup_lazy(x, c.w, c.wq, q); }      // x*c mod q in [0,2q), any x

// BEHZ steps 1-2 for one coefficient (L = nB = TL <= 3, Shoup-form matrices): xin = the L canonical q-limb residues,
// dst = limb 0 of the extended polynomial ([L q-limbs | nB B-limbs | m_sk][n]) at coefficient k.
template <int TL>
__device__ __forceinline__ void behz_ext2_body(const DevLevel *__restrict__ lv, const u64 *xin, u64 *__restrict__ dst, size_t n, size_t k)
{
    constexpr int L = TL, nBsk = TL + 1;
    u64 xs[L];
    u32 mt_acc = 0;
#pragma unroll
    for (int j = 0; j < L; j++) {
        const u64 x = xin[j];
        dst[(size_t)j * n + k] = x;
        xs[j] = mul_shoup(x, lv->ext_scale[j].w, lv->ext_scale[j].wq, lv->q[j].q);     // canonical: used as an integer
        mt_acc += (u32)xs[j] * lv->q_to_mt[j];
    }
    const u32 r32 = mt_acc * lv->neg_inv_q_mt;
#pragma unroll
    for (int i = 0; i < nBsk; i++) {
        const u64 m = lv->bsk[i].q;
        u64 r = r32;
        if (r32 >= 0x80000000u) r += m - ((u64)1 << 32);          // centred lift of r into Z_m
        // sm_mrq: (x_i + q r) m_tilde^-1 mod m with x_i = sum_j xs_j (Q/q_j): m_tilde^-1 is folded into both constants (round 4), so
        // the closing product is a reduction of the lazy sum v < (2L + 2) m <= 8 m < 2^64 -- the same residue, one Shoup product less
        u64 v = lazy2(r, lv->s_prod_q_bsk_mt[i], m);
#pragma unroll
        for (int j = 0; j < L; j++) v += lazy2(xs[j], lv->s_q_to_bsk_mt[i][j], m);
        dst[(size_t)(L + i) * n + k] = csub(csub(csub(v, m << 2), m << 1), m);
    }
}

// Fully unrolled variant for L = nB = TL <= 3 with Shoup-form matrices: same values, ~35 % fewer multiplies.
// DROP: the input is one level higher (TL + 1 limbs per polynomial) and is first mod-switched to this level
// (mod_switch_to_next_inplace, bin_bundle.cpp:269,298) — the drop and the extension share one pass over the data.
template <int TL, bool DROP, bool RAW = false>
__global__ __launch_bounds__(EW_T) void k_behz_ext2(const DevLevel *__restrict__ lv, const u64 *__restrict__ in,
                                                    size_t in_stride, int polys, u64 *__restrict__ out, size_t n)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    constexpr int L = TL, E = 2 * TL + 1, LIN = TL + (DROP ? 1 : 0);
    const size_t c = blockIdx.y / polys, p = blockIdx.y % polys;
    const u64 *src = in + c * in_stride + p * (size_t)LIN * n;
    u64 *dst = out + (size_t)blockIdx.y * E * n;
    u64 xin[L];
    if (DROP) {
        const DevLevel *ld = lv + 1;                              // constants of the level being left
        const u64 ql = ld->q[L].q;
        u64 lastc = src[(size_t)L * n + k];
        if (RAW) {                                                // the inverse transform left its twist to this kernel
            const u64x2 tw = ldg16(reinterpret_cast<const u64 *>(ld->last_tw + k));
            lastc = mul_shoup(lastc, tw[0], tw[1], ql);
        }
        const u64 last = addmod(lastc, ld->half, ql);
#pragma unroll
        for (int j = 0; j < L; j++) {
            const Mod m = ld->q[j];
            const u64 tmp = submod(barrett64(last, m), ld->half_mod[j], m.q);
            if (RAW) {
                // (c_j - tmp) q_last^-1 with c_j = raw_j * twist: two lazy products, the twist folded into the first constant
                const u64x2 tw = ldg16(reinterpret_cast<const u64 *>(ld->drop_tw[j] + k));
                const u64 a = mul_shoup_lazy(src[(size_t)j * n + k], tw[0], tw[1], m.q);                       // [0, 2q)
                const u64 b = mul_shoup_lazy(tmp, ld->inv_q_last[j].w, ld->inv_q_last[j].wq, m.q);           // [0, 2q)
                xin[j] = csub(csub(a + (m.q << 1) - b, m.q << 1), m.q);
            } else xin[j] = mul_shoup(submod(src[(size_t)j * n + k], tmp, m.q), ld->inv_q_last[j].w, ld->inv_q_last[j].wq, m.q);
        }
    } else {
#pragma unroll
        for (int j = 0; j < L; j++) xin[j] = src[(size_t)j * n + k];
    }
    behz_ext2_body<TL>(lv, xin, dst, n, k);
}

// drop one limb, then extend: `in` holds polynomials of L + 1 limbs at level lv + 1.  Only for the unrolled sizes;
// returns false when the caller has to run the two steps separately.
bool launch_drop_behz_ext(const DevLevel *lv, int L, int nB, const u64 *in, size_t in_stride, int polys, u64 *out, size_t n, int cts,
                          hipStream_t st, bool raw)
{
    if (!cts) return true;
    const dim3 g = ew_grid(n, cts * polys), t(EW_T);
#define EXT2_CASE(TL) if (behz_unrolled(L, nB) && L == TL) { \
        if (raw) hipLaunchKernelGGL((k_behz_ext2<TL, true, true>), g, t, 0, st, lv, in, in_stride, polys, out, n); \
        else hipLaunchKernelGGL((k_behz_ext2<TL, true>), g, t, 0, st, lv, in, in_stride, polys, out, n); \
        KERNEL_CHECK(); return true; }
    EXT2_CASE(1) EXT2_CASE(2) EXT2_CASE(3)
#undef EXT2_CASE
    return false;
}

void launch_behz_ext(const DevLevel *lv, int L, int nB, const u64 *in, size_t in_stride, int polys, u64 *out, size_t n, int cts,
                     hipStream_t st)
{
    if (!cts) return;
    const dim3 g = ew_grid(n, cts * polys), t(EW_T);
#define EXT2_CASE(TL) if (behz_unrolled(L, nB) && L == TL) { hipLaunchKernelGGL((k_behz_ext2<TL, false>), g, t, 0, st, lv, in, in_stride, polys, out, n); KERNEL_CHECK(); return; }
    EXT2_CASE(1) EXT2_CASE(2) EXT2_CASE(3)
#undef EXT2_CASE
    if (L == 4 && nB == 4) hipLaunchKernelGGL((k_behz_ext<4, 4>), g, t, 0, st, lv, in, in_stride, polys, out, n);
    else hipLaunchKernelGGL((k_behz_ext<0, 0>), g, t, 0, st, lv, in, in_stride, polys, out, n);
    KERNEL_CHECK();
}

// Step (4): tensor product in the NTT domain over all E limbs: d0=a0b0, d1=a0b1+a1b0, d2=a1b1
__global__ __launch_bounds__(EW_T) void k_tensor(const DevLevel *__restrict__ lv, const TensorJob *__restrict__ jobs, size_t n)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const TensorJob job = jobs[blockIdx.y];
    const int E = lv->E;
    const size_t ps = (size_t)E * n;
    for (int e = 0; e < E; e++) {
        const Mod m = lv->ext[e];
        const size_t o = e * n + k;
        const u64 a0 = job.a[o], a1 = job.a[ps + o], b0 = job.b[o], b1 = job.b[ps + o];
        job.d[o] = mulmod(a0, b0, m);
        u128p mid = mul128(a0, b1);
        mac128(mid, a1, b0);
        job.d[ps + o] = barrett128(mid, m);
        job.d[2 * ps + o] = mulmod(a1, b1, m);
    }
}

void launch_tensor(const DevLevel *lv, const TensorJob *jobs, size_t n, int batch, hipStream_t st)
{
    hipLaunchKernelGGL(k_tensor, ew_grid(n, batch), dim3(EW_T), 0, st, lv, jobs, n);
    KERNEL_CHECK();
}

// Step (4) for ciphertexts of any size (parameter sets without key switching never relinearise, receiver_osn.cpp:430-432, so
// operands keep growing): d_I = sum_{i + j = I} a_i b_j, limb-wise, every product reduced before the modular add
// (Evaluator::bfv_multiply's behz_ciphertext_product).  Not a hot path: no shipped parameter set reaches it.
__global__ __launch_bounds__(EW_T) void k_tensor_conv(const DevLevel *__restrict__ lv, const TensorConvJob *__restrict__ jobs, size_t n)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const TensorConvJob job = jobs[blockIdx.y];
    const int E = lv->E;
    const size_t ps = (size_t)E * n;
    const int so = job.sa + job.sb - 1;
    for (int e = 0; e < E; e++) {
        const Mod m = lv->ext[e];
        const size_t o = e * n + k;
        for (int I = 0; I < so; I++) {
            const int i0 = I - (job.sb - 1) > 0 ? I - (job.sb - 1) : 0, i1 = I < job.sa - 1 ? I : job.sa - 1;
            u64 acc = 0;
            for (int i = i0; i <= i1; i++) acc = addmod(acc, mulmod(job.a[i * ps + o], job.b[(I - i) * ps + o], m), m.q);
            job.d[I * ps + o] = acc;
        }
    }
}

void launch_tensor_conv(const DevLevel *lv, const TensorConvJob *jobs, size_t n, int njobs, hipStream_t st)
{
    if (!njobs) return;
    hipLaunchKernelGGL(k_tensor_conv, ew_grid(n, njobs), dim3(EW_T), 0, st, lv, jobs, n);
    KERNEL_CHECK();
}

// Step (4) for a SUM of products (eval_patstock's sum over i): the q limbs of every term are kept (their canonical
// coefficient-form residues are needed per term by the finish), the Bsk limbs are summed here in the NTT domain.
// e0 = L: only the Bsk sums (the per-term q limbs are formed by k_intt_tensor on load).
__global__ __launch_bounds__(EW_T) void k_tensor_sum(const DevLevel *__restrict__ lv, const TensorSumJob *__restrict__ jobs, size_t n, int e0)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const TensorSumJob job = jobs[blockIdx.z];
    const int E = lv->E, L = lv->L, e = blockIdx.y + e0;
    const size_t ps = (size_t)E * n, o = (size_t)e * n + k;
    const Mod m = lv->ext[e];
    if (e < L) {
        for (int i = 0; i < job.terms; i++) {
            const u64 *a = job.a + (size_t)i * 2 * ps, *b = job.b + (size_t)i * 2 * ps;
            const u64 a0 = a[o], a1 = a[ps + o], b0 = b[o], b1 = b[ps + o];
            u64 *d = job.dq + (size_t)i * 3 * L * n + o;
            d[0] = mulmod(a0, b0, m);
            u128p mid = mul128(a0, b1);
            mac128(mid, a1, b0);
            d[(size_t)L * n] = barrett128(mid, m);
            d[(size_t)2 * L * n] = mulmod(a1, b1, m);
        }
    } else {
        u128p s0{ 0, 0 }, s1{ 0, 0 }, s2{ 0, 0 };
        u64 r0 = 0, r1 = 0, r2 = 0;
        for (int i = 0; i < job.terms; i++) {
            const u64 *a = job.a + (size_t)i * 2 * ps, *b = job.b + (size_t)i * 2 * ps;
            const u64 a0 = a[o], a1 = a[ps + o], b0 = b[o], b1 = b[ps + o];
            mac128(s0, a0, b0);
            mac128(s1, a0, b1);
            mac128(s1, a1, b0);
            mac128(s2, a1, b1);
            if ((i & 7) == 7 || i + 1 == job.terms) {              // 16 products of < 2^62 bits each fit 128 bits
                r0 = addmod(r0, barrett128(s0, m), m.q);
                r1 = addmod(r1, barrett128(s1, m), m.q);
                r2 = addmod(r2, barrett128(s2, m), m.q);
                s0 = s1 = s2 = u128p{ 0, 0 };
            }
        }
        const int nBsk = E - L;
        u64 *d = job.bs + (size_t)(e - L) * n + k;
        d[0] = r0;
        d[(size_t)nBsk * n] = r1;
        d[(size_t)2 * nBsk * n] = r2;
    }
}

void launch_tensor_sum(const DevLevel *lv, int E, const TensorSumJob *jobs, size_t n, int njobs, int e0, hipStream_t st)
{
    if (!njobs || e0 >= E) return;
    hipLaunchKernelGGL(k_tensor_sum, dim3((unsigned)((n + EW_T - 1) / EW_T), E - e0, njobs), dim3(EW_T), 0, st, lv, jobs, n, e0);
    KERNEL_CHECK();
}

// Steps (6)-(8) for one coefficient of one extended polynomial: multiply by t, fast_floor
// (q u Bsk -> Bsk), fastbconv_sk (Bsk -> q).  d points at limb 0 of the polynomial, stride n.
//
// `terms` > 1 finishes a SUM of products in one go (eval_patstock's sum over i, bin_bundle.cpp:273,303): dq holds the q
// limbs of every term (stride term_stride), dbsk the Bsk limbs of the sum.  The only per-term non-linearity of
// steps (6)-(8) is the canonical residue [t d (Q/q_j)^-1]_{q_j} feeding fastbconv(q -> Bsk); those residues are
// summed as integers, everything after is linear mod Bsk_i and fastbconv_sk is exact, so the result equals the
// sum of the individually finished terms bit for bit (note N1).
template <int TL, int TNB>
__device__ __forceinline__ void behz_finish_coeff(const DevLevel *__restrict__ lv, const u64 *__restrict__ dq, size_t term_stride,
                                                  int terms, const u64 *__restrict__ dbsk, size_t n, u64 *res /* [L] */)
{
    const int L = TL ? TL : lv->L, nB = TL ? TNB : lv->nB, nBsk = nB + 1;
    constexpr int LMAX = TL ? TL : DMAXL;
    constexpr int BMAX = TL ? TNB + 1 : DMAXB;
    u64 xq[LMAX];
#pragma unroll
    for (int j = 0; j < LMAX; j++) xq[j] = 0;
    for (int it = 0; it < terms; it++) {
#pragma unroll
        for (int j = 0; j < LMAX; j++)                           // terms * q_j < 2^64 (host-checked)
            if (TL || j < L) xq[j] += mul_shoup(dq[it * term_stride + (size_t)j * n], lv->t_inv_punct_q[j].w, lv->t_inv_punct_q[j].wq, lv->q[j].q);
    }
    u64 ys[BMAX];
    u64 fl_sk = 0;
#pragma unroll
    for (int i = 0; i < BMAX; i++) {
        if (TL || i < nBsk) {
            const Mod m = lv->bsk[i];
            u128p acc{ 0, 0 };
#pragma unroll
            for (int j = 0; j < LMAX; j++)
                if (TL || j < L) mac128(acc, xq[j], lv->q_to_bsk[i][j]);
            const u64 conv = barrett128(acc, m);
            const u64 xb = mul_shoup(dbsk[(size_t)i * n], lv->t_bsk[i].w, lv->t_bsk[i].wq, m.q);
            const u64 fl = mul_shoup(xb + (m.q - conv), lv->inv_prod_q_bsk[i].w, lv->inv_prod_q_bsk[i].wq, m.q);
            if (i < nB) ys[i] = mul_shoup(fl, lv->inv_punct_B[i].w, lv->inv_punct_B[i].wq, m.q);
            else fl_sk = fl;
        }
    }
    const Mod msk = lv->bsk[nB];
    u128p acc{ 0, 0 };
#pragma unroll
    for (int i = 0; i < BMAX - 1; i++)
        if (TL || i < nB) mac128(acc, ys[i], lv->B_to_msk[i]);
    const u64 z_sk = barrett128(acc, msk);
    const u64 alpha = mul_shoup(z_sk + (msk.q - fl_sk), lv->inv_prod_B_msk.w, lv->inv_prod_B_msk.wq, msk.q);
    const bool neg = alpha > lv->msk_half;                     // alpha represents a negative value
    const u64 a_abs = neg ? msk.q - alpha : alpha;
#pragma unroll
    for (int j = 0; j < LMAX; j++) {
        if (TL || j < L) {
            u128p z{ 0, 0 };
#pragma unroll
            for (int i = 0; i < BMAX - 1; i++)
                if (TL || i < nB) mac128(z, ys[i], lv->B_to_q[j][i]);
            mac128(z, a_abs, neg ? lv->prod_B_q[j] : lv->neg_prod_B_q[j]);
            res[j] = barrett128(z, lv->q[j]);
        }
    }
}

// One job = one output polynomial triple: out[3][L][n] (+)= sum over `terms` consecutive extended
// products d[term][3][E][n] (coefficient form).  The per-term rounding is kept (SURVEY note N1).
template <int TL, int TNB>
__global__ __launch_bounds__(EW_T) void k_behz_finish(const DevLevel *__restrict__ lv, const FinishJob *__restrict__ jobs,
                                                      int accumulate, size_t n)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const int L = TL ? TL : lv->L, E = TL ? 2 * TL + 1 + (TNB - TL) : lv->E;
    constexpr int LMAX = TL ? TL : DMAXL;
    const FinishJob job = jobs[blockIdx.y / 3];
    const size_t p = blockIdx.y % 3;
    u64 sum[LMAX];
    u64 *o = job.out + p * (size_t)L * n + k;
#pragma unroll
    for (int j = 0; j < LMAX; j++)
        if (TL || j < L) sum[j] = accumulate ? o[(size_t)j * n] : 0;
    for (int i = 0; i < job.terms; i++) {
        const u64 *dp = job.d + (((size_t)i * 3 + p) * (size_t)E) * n + k;
        u64 res[LMAX];
        behz_finish_coeff<TL, TNB>(lv, dp, 0, 1, dp + (size_t)L * n, n, res);
#pragma unroll
        for (int j = 0; j < LMAX; j++)
            if (TL || j < L) sum[j] = addmod(sum[j], res[j], lv->q[j].q);
    }
#pragma unroll
    for (int j = 0; j < LMAX; j++)
        if (TL || j < L) o[(size_t)j * n] = sum[j];
}

// Fully unrolled variant for L = nB = TL <= 3 with Shoup-form matrices (same values as behz_finish_coeff).
// dq / dbsk come from an inverse NTT that left out its twist (NTT_MAP_RAW): raw lazy values, any 64-bit number; the twist
// is part of the per-position constants fin_q / fin_b (kidx = coefficient index).
// The level constants of the unrolled finish (four conversion rows of Shoup pairs, ...) are ~100 scalar registers when the compiler
// hoists every load to the top of the kernel: it then spills scalar registers into vector lanes (v_writelane / v_readlane, 16 % of
// the instructions of k_behz_finish2<3>).  A compiler-level memory fence per output row keeps each row's loads next to their use.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(APSU_FIN_NO_FENCE)
#define FIN_LOAD_FENCE() asm volatile("" ::: "memory")
#else
#define FIN_LOAD_FENCE() do { } while (0)
#endif
template <int TL>
__device__ __forceinline__ void behz_finish_coeff2(const DevLevel *__restrict__ lv, const u64 *__restrict__ dq, size_t term_stride,
                                                   int terms, const u64 *__restrict__ dbsk, size_t n, u64 *res, size_t kidx)
{
    constexpr int L = TL, nB = TL, nBsk = TL + 1;
    u64 xq[L];
#pragma unroll
    for (int j = 0; j < L; j++) xq[j] = 0;
    ShoupConst cq[L];
#pragma unroll
    for (int j = 0; j < L; j++) { const u64x2 v = ldg16(reinterpret_cast<const u64 *>(lv->fin_q[j] + kidx)); cq[j] = ShoupConst{ v[0], v[1] }; }
    for (int it = 0; it < terms; it++) {
#pragma unroll
        for (int j = 0; j < L; j++)                              // canonical: used as integers by the base conversion
            xq[j] += mul_shoup(dq[it * term_stride + (size_t)j * n], cq[j].w, cq[j].wq, lv->q[j].q);
    }
    u64 ys[nB];
    u64 fl_sk = 0;
#pragma unroll
    for (int i = 0; i < nBsk; i++) {
        FIN_LOAD_FENCE();
        const u64 m = lv->bsk[i].q;
        u64 conv = 0;                                            // < 2 L m
#pragma unroll
        for (int j = 0; j < L; j++) conv += lazy2(xq[j], lv->s_q_to_bsk[i][j], m);
        const u64x2 cb = ldg16(reinterpret_cast<const u64 *>(lv->fin_b[i] + kidx));
        const u64 xb = lazy2(dbsk[(size_t)i * n], ShoupConst{ cb[0], cb[1] }, m);
        const u64 diff = xb + ((u64)(2 * L) * m - conv);         // < (2L + 2) m <= 8 m < 2^64
        const u64 f = mul_shoup(diff, lv->s_fl[i].w, lv->s_fl[i].wq, m);      // i < nB: already times (B/b_i)^-1
        if (i < nB) ys[i] = f; else fl_sk = f;
    }
    const u64 msk = lv->bsk[nB].q;
    u64 z_sk = msk - fl_sk;                                      // (z - fl_sk) mod m_sk, lazily
#pragma unroll
    for (int i = 0; i < nB; i++) z_sk += lazy2(ys[i], lv->s_B_to_msk[i], msk);
    const u64 alpha = mul_shoup(z_sk, lv->inv_prod_B_msk.w, lv->inv_prod_B_msk.wq, msk);
    const bool neg = alpha > lv->msk_half;
    const u64 a_abs = neg ? msk - alpha : alpha;
#pragma unroll
    for (int j = 0; j < L; j++) {
        FIN_LOAD_FENCE();
        const u64 q = lv->q[j].q;
        u64 z = lazy2(a_abs, neg ? lv->s_prod_B_q[j] : lv->s_neg_prod_B_q[j], q);       // < (2 nB + 2) q <= 8 q
#pragma unroll
        for (int i = 0; i < nB; i++) z += lazy2(ys[i], lv->s_B_to_q[j][i], q);
        res[j] = csub(csub(csub(z, q << 2), q << 1), q);
    }
}

template <int TL>
__global__ __launch_bounds__(EW_T) void k_behz_finish2(const DevLevel *__restrict__ lv, const FinishJob *__restrict__ jobs,
                                                       int accumulate, size_t n)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    constexpr int L = TL, E = 2 * TL + 1;
    const FinishJob job = jobs[blockIdx.y / 3];
    const size_t p = blockIdx.y % 3;
    u64 sum[L];
    u64 *o = job.out + p * (size_t)L * n + k;
#pragma unroll
    for (int j = 0; j < L; j++) sum[j] = accumulate ? o[(size_t)j * n] : 0;
    for (int i = 0; i < job.terms; i++) {
        u64 res[L];
        const u64 *dp = job.d + (((size_t)i * 3 + p) * (size_t)E) * n + k;
        behz_finish_coeff2<TL>(lv, dp, 0, 1, dp + (size_t)L * n, n, res, k);
#pragma unroll
        for (int j = 0; j < L; j++) sum[j] = addmod(sum[j], res[j], lv->q[j].q);
    }
#pragma unroll
    for (int j = 0; j < L; j++) o[(size_t)j * n] = sum[j];
}

void launch_behz_finish(const DevLevel *lv, int L, int nB, const FinishJob *jobs, bool accumulate, size_t n, int njobs, hipStream_t st)
{
    if (!njobs) return;
    const dim3 g = ew_grid(n, njobs * 3), t(EW_T);
    const int acc = accumulate ? 1 : 0;
#define FIN2_CASE(TL) if (behz_unrolled(L, nB) && L == TL) { hipLaunchKernelGGL((k_behz_finish2<TL>), g, t, 0, st, lv, jobs, acc, n); KERNEL_CHECK(); return; }
    FIN2_CASE(1) FIN2_CASE(2) FIN2_CASE(3)
#undef FIN2_CASE
    if (L == 4 && nB == 4) hipLaunchKernelGGL((k_behz_finish<4, 4>), g, t, 0, st, lv, jobs, acc, n);
    else hipLaunchKernelGGL((k_behz_finish<0, 0>), g, t, 0, st, lv, jobs, acc, n);
    KERNEL_CHECK();
}

// Finish of a summed product: one job = one BinBundle; out[3][L][n] = sum over terms of the finished products.
template <int TL, bool LAZY>
__global__ __launch_bounds__(EW_T) void k_behz_finish_sum(const DevLevel *__restrict__ lv, const FinishSumJob *__restrict__ jobs, size_t n)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const int L = TL ? TL : lv->L, nBsk = TL ? TL + 1 : lv->nBsk;
    constexpr int LMAX = TL ? TL : DMAXL;
    const FinishSumJob job = jobs[blockIdx.y / 3];
    const size_t p = blockIdx.y % 3;
    const u64 *dq = job.dq + p * (size_t)L * n + k;
    const u64 *db = job.bs + p * (size_t)nBsk * n + k;
    u64 res[LMAX];
    if constexpr (LAZY) behz_finish_coeff2<TL>(lv, dq, (size_t)3 * L * n, job.terms, db, n, res, k);
    else behz_finish_coeff<TL, TL>(lv, dq, (size_t)3 * L * n, job.terms, db, n, res);
    u64 *o = job.out + p * (size_t)L * n + k;
#pragma unroll
    for (int j = 0; j < LMAX; j++)
        if (TL || j < L) o[(size_t)j * n] = res[j];
}

void launch_behz_finish_sum(const DevLevel *lv, int L, int nB, const FinishSumJob *jobs, size_t n, int njobs, hipStream_t st)
{
    if (!njobs) return;
    const dim3 g = ew_grid(n, njobs * 3), t(EW_T);
#define FS_CASE(TL) if (behz_unrolled(L, nB) && L == TL) { hipLaunchKernelGGL((k_behz_finish_sum<TL, true>), g, t, 0, st, lv, jobs, n); KERNEL_CHECK(); return; }
    FS_CASE(1) FS_CASE(2) FS_CASE(3)
#undef FS_CASE
    if (L == 4 && nB == 4) hipLaunchKernelGGL((k_behz_finish_sum<4, false>), g, t, 0, st, lv, jobs, n);
    else hipLaunchKernelGGL((k_behz_finish_sum<0, false>), g, t, 0, st, lv, jobs, n);
    KERNEL_CHECK();
}

// ============================================================================ K6: relinearize (key switch of c2)
// relinearize_inplace (receiver_osn.cpp:431 ; bin_bundle.cpp:309), App. B10.
// The RNS decomposition c2[J] mod m_I is done by k_ntt_gather on load (no separate pass).
// inner product with the key: acc[b][comp][I][k] = sum_J tdec[b][I][J][k] * rk[J][comp][id(I)][k] mod m_I
template <int TL>
__global__ __launch_bounds__(EW_T) void k_ks_inner(const DevKey *__restrict__ key, int Lrt, const u64 *__restrict__ tdec,
                                                   const u64 *__restrict__ rk, u64 *__restrict__ acc, size_t n)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const size_t b = blockIdx.y;
    const int L = TL ? TL : Lrt;
    const int K = key->K;
    const u64 *td = tdec + b * (size_t)(L + 1) * L * n;
    u64 *o = acc + b * (size_t)2 * (L + 1) * n;
#pragma unroll
    for (int I = 0; I <= (TL ? TL : DMAXL); I++) {
        if (!TL && I > L) continue;
        const int ki = I == L ? K - 1 : I;
        const Mod m = key->q[ki];
        u128p a0{ 0, 0 }, a1{ 0, 0 };
#pragma unroll
        for (int J = 0; J < (TL ? TL : DMAXL); J++) {
            if (!TL && J >= L) continue;
            const u64 tv = td[((size_t)I * L + J) * n + k];
            mac128(a0, tv, rk[(((size_t)J * 2 + 0) * K + ki) * n + k]);
            mac128(a1, tv, rk[(((size_t)J * 2 + 1) * K + ki) * n + k]);
        }
        o[(size_t)I * n + k] = barrett128(a0, m);
        o[((size_t)(L + 1) + I) * n + k] = barrett128(a1, m);
    }
}

void launch_ks_inner(const DevKey *key, int L, const u64 *tdec, const u64 *rk, u64 *acc, size_t n, int batch,
                     hipStream_t st)
{
#define KS_CASE(TL) case TL: hipLaunchKernelGGL((k_ks_inner<TL>), ew_grid(n, batch), dim3(EW_T), 0, st, key, L, tdec, rk, acc, n); break;
    switch (L) { KS_CASE(1) KS_CASE(2) KS_CASE(3) KS_CASE(4) default: hipLaunchKernelGGL((k_ks_inner<0>), ew_grid(n, batch), dim3(EW_T), 0, st, key, L, tdec, rk, acc, n); }
#undef KS_CASE
    KERNEL_CHECK();
}

// mod-down by the special prime with rounding and add into (c0, c1):
// acc: [batch][2][L+1][n] coefficient form ; ct[b]: [>=2][L][n] at stride ct_stride
// EXT: the first n_ext ciphertexts are operands of later products (ComputePowers' parents): their BEHZ extension
// (steps 1-2, behz_ext2_body) is written to ext + (b*2 + comp)*(2L+1)*n while the new (c0, c1) are still in registers --
// the extension kernel of the next DAG level and its re-read of the ciphertexts disappear.
template <int TL, bool EXT = false, bool RAW = false>
__global__ __launch_bounds__(EW_T) void k_ks_moddown(const DevKey *__restrict__ key, int Lrt, const u64 *__restrict__ acc,
                                                     u64 *__restrict__ ct, size_t ct_stride, size_t n,
                                                     const DevLevel *__restrict__ lv = nullptr, u64 *__restrict__ ext = nullptr, int n_ext = 0)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const size_t b = blockIdx.y;
    const int L = TL ? TL : Lrt;
    const Mod pm = key->q[key->K - 1];
#pragma unroll
    for (int comp = 0; comp < 2; comp++) {
        const u64 *a = acc + (b * 2 + comp) * (size_t)(L + 1) * n;
        u64 *c = ct + b * ct_stride + (size_t)comp * L * n;
        u64 ap = a[(size_t)L * n + k];
        if (RAW) {                                                // RAW: the inverse transform left its twist to this kernel
            const u64x2 tw = ldg16(reinterpret_cast<const u64 *>(key->p_tw + k));
            ap = mul_shoup(ap, tw[0], tw[1], pm.q);
        }
        const u64 tl = barrett64(ap + key->p_half, pm);
        u64 x[TL ? TL : 1];
#pragma unroll
        for (int j = 0; j < (TL ? TL : DMAXL); j++) {
            if (!TL && j >= L) continue;
            const Mod m = key->q[j];
            const u64 tk = submod(barrett64(tl, m), key->p_half_mod[j], m.q);
            u64 v;
            if (RAW) {
                const u64x2 tw = ldg16(reinterpret_cast<const u64 *>(key->md_tw[j] + k));
                const u64 u = mul_shoup_lazy(a[(size_t)j * n + k], tw[0], tw[1], m.q);                         // [0, 2q)
                const u64 w = mul_shoup_lazy(tk, key->inv_p[j].w, key->inv_p[j].wq, m.q);                     // [0, 2q)
                v = csub(csub(u + (m.q << 1) - w, m.q << 1), m.q);
            } else v = mul_shoup(submod(a[(size_t)j * n + k], tk, m.q), key->inv_p[j].w, key->inv_p[j].wq, m.q);
            const u64 r = addmod(c[(size_t)j * n + k], v, m.q);
            c[(size_t)j * n + k] = r;
            if (EXT) x[j] = r;
        }
        if constexpr (EXT && TL > 0) {
            if ((int)b < n_ext) behz_ext2_body<TL>(lv, x, ext + ((b * 2 + comp) * (size_t)(2 * TL + 1)) * n, n, k);
        }
    }
}

// lv / ext / n_ext: see k_ks_moddown<TL, true>; only for L == nB <= 3 (the caller checks), ext == nullptr: plain mod-down
void launch_ks_moddown(const DevKey *key, int L, const u64 *acc, u64 *ct, size_t ct_stride, size_t n, int batch,
                       hipStream_t st, const DevLevel *lv, u64 *ext, int n_ext, bool raw)
{
    const dim3 g = ew_grid(n, batch), t(EW_T);
    if (ext && n_ext > 0 && L >= 1 && L <= 3) {
#define KSX_CASE(TL) case TL: if (raw) hipLaunchKernelGGL((k_ks_moddown<TL, true, true>), g, t, 0, st, key, L, acc, ct, ct_stride, n, lv, ext, n_ext); \
                              else hipLaunchKernelGGL((k_ks_moddown<TL, true>), g, t, 0, st, key, L, acc, ct, ct_stride, n, lv, ext, n_ext); break;
        switch (L) { KSX_CASE(1) KSX_CASE(2) KSX_CASE(3) }
#undef KSX_CASE
        KERNEL_CHECK();
        return;
    }
    if (raw && (L < 1 || L > 4)) throw_hip(hipErrorInvalidValue, __FILE__, __LINE__);
#define KS_CASE(TL) case TL: if (raw) hipLaunchKernelGGL((k_ks_moddown<TL, false, true>), g, t, 0, st, key, L, acc, ct, ct_stride, n, nullptr, nullptr, 0); \
                             else hipLaunchKernelGGL((k_ks_moddown<TL>), g, t, 0, st, key, L, acc, ct, ct_stride, n, nullptr, nullptr, 0); break;
    switch (L) { KS_CASE(1) KS_CASE(2) KS_CASE(3) KS_CASE(4) default: hipLaunchKernelGGL((k_ks_moddown<0>), g, t, 0, st, key, L, acc, ct, ct_stride, n, nullptr, nullptr, 0); }
#undef KS_CASE
    KERNEL_CHECK();
}

// Fused tail of BatchedPlaintextPolyn::eval / eval_patstock (bin_bundle.cpp:159-171, 345-357):
// add_plain(a_0), add_plain(random_plain) [K8], mod_switch_to_next down to the last level [K7],
// try_clear_irrelevant_bits [K9] — plus up to two exact addends (coefficient-form sums) folded in.
__device__ __forceinline__ u64 scaled_plain(const DevLevel *__restrict__ lv, u64 m, u64 fix, int j)
{
    u128p s = mul128(m, lv->coeff_div_plain[j]);
    add128(s, u128p{ fix, 0 });
    return barrett128(s, lv->q[j]);
}
__device__ __forceinline__ u64 plain_fix(const DevLevel *__restrict__ lv, u64 m)
{
    // floor((m * (Q mod t) + floor((t+1)/2)) / t), exact (m < t < 2^61)
    u128p num = mul128(m, lv->q_mod_t);
    add128(num, u128p{ lv->threshold, 0 });
    const u64 t = lv->t;
    if (num.hi == 0) return num.lo / t;
    u64 rem = num.hi % t, lo = num.lo, fix = 0;
    for (int i = 0; i < 64; i++) {
        rem = (rem << 1) | (lo >> 63);
        lo <<= 1;
        fix <<= 1;
        if (rem >= t) { rem -= t; fix |= 1; }
    }
    return fix;
}

// MD (round 6): the key switch's mod-down (k_ks_moddown<., false, RAW>, App. B10) runs HERE, on the way in: job.ks_acc = the RAW inverse
// transforms of the key-switch sums [2][L+1][n]; (c0, c1) + the rounded quotient never goes to memory and the mod-down launch in front
// of this kernel is gone (one launch and one boundary per query: -6 us on the N = 8 shard's critical path, profiles/r06_ab_fused_tail.txt).
template <bool MD>
__global__ __launch_bounds__(EW_T) void k_eval_epilogue(const DevLevel *__restrict__ levels, int lvl, const EpiJob *__restrict__ jobs,
                                                        size_t ct_poly_stride, u64 clear_mask, size_t n, const DevKey *__restrict__ key)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const EpiJob job = jobs[blockIdx.y];
    const DevLevel *lv = levels + lvl;
    const int L = lvl + 1;
    u64 v[2][DMAXL];
#pragma unroll
    for (int p = 0; p < 2; p++) {
        u64 tl = 0;
        const u64 *a = nullptr;
        if constexpr (MD) {                                      // the special limb of this polynomial's key-switch sum, twisted and rounded
            a = job.ks_acc + (size_t)p * (L + 1) * n;
            const Mod pm = key->q[key->K - 1];
            const u64x2 tw = ldg16(reinterpret_cast<const u64 *>(key->p_tw + k));
            tl = barrett64(mul_shoup(a[(size_t)L * n + k], tw[0], tw[1], pm.q) + key->p_half, pm);
        }
#pragma unroll
        for (int j = 0; j < DMAXL; j++)
            if (j < L) {
                const u64 q = lv->q[j].q;
                u64 x = job.ct[p * ct_poly_stride + (size_t)j * n + k];
                if constexpr (MD) {                              // exactly k_ks_moddown's RAW arithmetic
                    const Mod m = key->q[j];
                    const u64 tk = submod(barrett64(tl, m), key->p_half_mod[j], m.q);
                    const u64x2 tw = ldg16(reinterpret_cast<const u64 *>(key->md_tw[j] + k));
                    const u64 u = mul_shoup_lazy(a[(size_t)j * n + k], tw[0], tw[1], m.q);
                    const u64 w = mul_shoup_lazy(tk, key->inv_p[j].w, key->inv_p[j].wq, m.q);
                    x = addmod(x, csub(csub(u + (m.q << 1) - w, m.q << 1), m.q), m.q);
                }
                if (job.add1) x = addmod(x, job.add1[((size_t)p * L + j) * n + k], q);
                if (job.add2) x = addmod(x, job.add2[((size_t)p * L + j) * n + k], q);
                v[p][j] = x;
            }
    }
    {   // c0 += round(a0 * Q / t) + round(mask * Q / t)
        const u64 m0 = job.a0[k], m1 = job.mask[k];
        const u64 f0 = plain_fix(lv, m0), f1 = plain_fix(lv, m1);
#pragma unroll
        for (int j = 0; j < DMAXL; j++)
            if (j < L) {
                const u64 q = lv->q[j].q;
                v[0][j] = addmod(addmod(v[0][j], scaled_plain(lv, m0, f0, j), q), scaled_plain(lv, m1, f1, j), q);
            }
    }
    for (int l = lvl; l > 0; l--) {                              // drop q_l with rounding (App. B8)
        const DevLevel *ll = levels + l;
        const u64 ql = ll->q[l].q;
#pragma unroll
        for (int p = 0; p < 2; p++) {
            u64 last = 0;
#pragma unroll
            for (int j = 0; j < DMAXL; j++) if (j == l) last = v[p][j];
            last = addmod(last, ll->half, ql);
#pragma unroll
            for (int j = 0; j < DMAXL; j++)
                if (j < l) {
                    const Mod m = ll->q[j];
                    const u64 tmp = submod(barrett64(last, m), ll->half_mod[j], m.q);
                    v[p][j] = mul_shoup(submod(v[p][j], tmp, m.q), ll->inv_q_last[j].w, ll->inv_q_last[j].wq, m.q);
                }
        }
    }
    job.out[k] = v[0][0] & clear_mask;
    job.out[n + k] = v[1][0] & clear_mask;
}

// key != nullptr: every job carries ks_acc and the key switch's mod-down is part of this launch (k_eval_epilogue<true>)
void launch_eval_epilogue(const DevLevel *levels, int lvl, const EpiJob *jobs, size_t ct_poly_stride, int clear_bits, size_t n,
                          int njobs, hipStream_t st, const DevKey *key)
{
    if (!njobs) return;
    const u64 mask = clear_bits > 0 ? ~(((u64)1 << clear_bits) - 1) : ~(u64)0;
    if (key) hipLaunchKernelGGL(k_eval_epilogue<true>, ew_grid(n, njobs), dim3(EW_T), 0, st, levels, lvl, jobs, ct_poly_stride, mask, n, key);
    else hipLaunchKernelGGL(k_eval_epilogue<false>, ew_grid(n, njobs), dim3(EW_T), 0, st, levels, lvl, jobs, ct_poly_stride, mask, n, key);
    KERNEL_CHECK();
}

// Sum of `terms` individually rounded drop-last-limb results, computed from the exact sum S of the kept
// limbs and the per-term last limbs V (all coefficient form):  SURVEY note N1 / DESIGN.md §4.
template <bool RAW>
__global__ __launch_bounds__(EW_T) void k_i0_finish(const DevLevel *__restrict__ lv, const I0Job *__restrict__ jobs, size_t n)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const I0Job job = jobs[blockIdx.y >> 1];
    const int p = blockIdx.y & 1;
    const int L = lv->L;                                        // level BEFORE the drop
    const u64 ql = lv->q[L - 1].q, half = lv->half;
    u64 R = 0;                                                  // integer sum of (v + half) mod q_last; terms*q_last < 2^64 (host-checked)
    const u64 *v = job.v + (size_t)p * n + k;
    u64 tw0 = 0, tw1 = 0;
    if (RAW) { const u64x2 tw = ldg16(reinterpret_cast<const u64 *>(lv->last_tw + k)); tw0 = tw[0]; tw1 = tw[1]; }
    for (int t = 0; t < job.terms; t++) {
        u64 x = v[(size_t)t * 2 * n];
        if (RAW) x = mul_shoup(x, tw0, tw1, ql);                // RAW: the inverse transform left its twist to this kernel
        R += addmod(x, half, ql);
    }
    for (int m = 0; m + 1 < L; m++) {
        const Mod mq = lv->q[m];
        // terms * (half mod q_m) - (R mod q_m)
        const u64 th = barrett128(mul128((u64)job.terms, lv->half_mod[m]), mq);
        const u64 corr = submod(th, barrett64(R, mq), mq.q);
        const size_t o = ((size_t)p * (L - 1) + m) * n + k;
        u64 r;
        if (RAW) {
            // (s + corr) q_last^-1 with s = raw * twist: the twist rides on the first product's constant
            const u64x2 tw = ldg16(reinterpret_cast<const u64 *>(lv->drop_tw[m] + k));
            const u64 a = mul_shoup_lazy(job.s[o], tw[0], tw[1], mq.q);                                         // [0, 2q)
            const u64 b = mul_shoup_lazy(corr, lv->inv_q_last[m].w, lv->inv_q_last[m].wq, mq.q);              // [0, 2q)
            r = csub(csub(a + b, mq.q << 1), mq.q);
        } else {
            const u64 val = addmod(job.s[o], corr, mq.q);
            r = mul_shoup(val, lv->inv_q_last[m].w, lv->inv_q_last[m].wq, mq.q);
        }
        job.acc[o] = job.store ? r : addmod(job.acc[o], r, mq.q);
    }
}

void launch_i0_finish(const DevLevel *lv_low, const I0Job *jobs, size_t n, int njobs, hipStream_t st, bool raw)
{
    if (!njobs) return;
    if (raw) hipLaunchKernelGGL(k_i0_finish<true>, ew_grid(n, njobs * 2), dim3(EW_T), 0, st, lv_low, jobs, n);
    else hipLaunchKernelGGL(k_i0_finish<false>, ew_grid(n, njobs * 2), dim3(EW_T), 0, st, lv_low, jobs, n);
    KERNEL_CHECK();
}

} // namespace apsu_he
