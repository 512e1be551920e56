// The element-wise kernels of the query-evaluation engine for gfx950: the tier-1 steps on ciphertexts (K3 single term, K4, K7-K10),
// copies and the source check, fills and seed expansion, the decryption's rounding step and the querier's side (query_side.h).
// One thread per coefficient; conventions in kernel_launch.h.
#include "launch_ew.h"
#include "kernel_launch.h"
#include "blake2x.h"
#include "query_side.h"
#include <algorithm>

namespace apsu_he {

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

// K8: add_plain_inplace (bin_bundle.cpp:159,162,345,346): c0 += round(m*Q/t) in RNS  (App. B7)
__global__ __launch_bounds__(EW_T) void k_add_plain(const DevLevel *__restrict__ lv, const PlainJob *__restrict__ jobs, size_t n)
{
    const size_t k = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (k >= n) return;
    const PlainJob job = jobs[blockIdx.y];
    const u64 m = job.pt[k];
    const u64 fix = plain_fix(lv, m);
    u64 *c0 = job.ct;
    for (int j = 0; j < lv->L; j++) {
        const u64 scaled = scaled_plain(lv, m, fix, j);
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
// cap (1 .. SEED_REJ_CAP, dev_consts.h): the positions an object's list takes; the list stride and the LDS array stay as compiled.
__global__ __launch_bounds__(EW_T) void k_seed_bulk(const SeedJob *__restrict__ jobs, const DevLevel *__restrict__ lv, const u64 *__restrict__ max_multiple,
                                                    size_t n, u32 *__restrict__ rej, u32 cap)
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
            if (slot < cap) list[1 + slot] = (u32)w;
        } else job.dst[w] = barrett64(blk[i], lv->q[j]);
    }
}

__global__ __launch_bounds__(64) void k_seed_fix(const SeedJob *__restrict__ jobs, const DevLevel *__restrict__ lv, const u64 *__restrict__ max_multiple,
                                                 size_t n, u32 *__restrict__ rej, u32 cap, int *__restrict__ overflow)
{
    __shared__ u32 sorted[SEED_REJ_CAP];
    __shared__ u64 cache[64 * 8];
    const SeedJob job = jobs[blockIdx.x];
    u32 *list = rej + (size_t)blockIdx.x * (1 + SEED_REJ_CAP);
    const u32 cnt = list[0];
    const u32 lane = threadIdx.x;
    if (cnt > cap) { if (lane == 0) *overflow = 1; return; }
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

void launch_seed_expand(const SeedJob *jobs, int njobs, const DevLevel *lv, int L, const u64 *max_multiple, size_t n, u32 *rej, u32 cap, int *overflow,
                        hipStream_t st)
{
    if (!njobs) return;
    const u64 blocks = ((u64)L * n + 7) / 8;
    hipLaunchKernelGGL(k_seed_bulk, dim3((unsigned)((blocks + EW_T - 1) / EW_T), (unsigned)njobs), dim3(EW_T), 0, st, jobs, lv, max_multiple, n, rej, cap);
    hipLaunchKernelGGL(k_seed_fix, dim3((unsigned)njobs), dim3(64), 0, st, jobs, lv, max_multiple, n, rej, cap, overflow);
    KERNEL_CHECK();
}

// N4: the querier's decryption of a result at the last level (result_package.cpp:175-213, Decryptor::decrypt):
// x = c0 + v (v = INTT(NTT(c1) . s), one limb q0), m = round(t x / q0) mod t.
// (decrypt_round_coeff: query_side.h)
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
// largest centred |t x mod q0| over ciphertext b's coefficients; the budget -- the largest b with worst 2^b < q0, i.e.
// ceil(log2(q0 / (2 worst))), and the bit count of q0 for worst = 0 -- is formed on the host.
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
    const u64 fix = plain_fix(lv, m);
    const int ek = e[c * n + k];
    const u64 *vc = v + c * L * n;
    u64 *c0 = cts + c * 2 * L * n;
    for (int j = 0; j < L; j++) {
        const u64 q = lv->q[j].q;
        const u64 x = submod(scaled_plain(lv, m, fix, j), qs_residue(ek, q), q);
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

} // namespace apsu_he
