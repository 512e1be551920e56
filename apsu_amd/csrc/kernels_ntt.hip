// The transforms of the query-evaluation engine for gfx950: k_ntt, the first and last stage of the split transform, k_ntt_gather and
// k_intt_tensor, their form tables and launchers.  ONE translation unit on purpose: the three kernel families share ntt_body and the pass
// functions (ntt_wg.h, ntt_core.h), and compiled apart 34 of the 40 kernels come out as another instruction stream.
// Kernels and table rows keep their order: it is the kernels' order in the code object.
#include "launch_ntt.h"
#include "kernel_launch.h"
#include "ntt_wg.h"
#include "ntt_form.h"
#include <type_traits>

namespace apsu_he {

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

} // namespace apsu_he
