// BFV multiply (BEHZ extension, tensor products, finish), the key switch, the fused tail of the evaluation and the i = 0 block's finish
// for gfx950.  One thread per coefficient; conventions in kernel_launch.h.
#include "launch_behz.h"
#include "kernel_launch.h"
#include "eval_plan.h"

namespace apsu_he {

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
