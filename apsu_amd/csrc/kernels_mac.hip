// K3: the dyadic multiply-accumulate family for gfx950, a translation unit of its own.  The inner loops of BatchedPlaintextPolyn::eval /
// eval_patstock (bin_bundle.cpp:140-149, 250-265, 279-294, 314-324, 328-337): out_g = sum_j C^j (.) a_{g,j} in the NTT domain for plaintext
// streams that share the same ciphertext powers (the inner polynomials of the BinBundles of one bundle index).  The HBM-resident plaintexts
// are streamed exactly once (16-byte non-temporal loads); every power load is shared by MAC_G streams.  The arithmetic is in mac_core.h,
// which the CPU tier runs as well: k_mac is the function defined there, the other kernels call theirs.
#include "launch_mac.h"
#include "kernel_launch.h"
#include <algorithm>

namespace apsu_he {

// (k_mac is defined in mac_core.h AS the kernel.  Do not wrap its body in a kernel here without comparing the gfx950 assembly with the
//  recorded one again: a called body compiles to another instruction stream, profiles/r13_mac_core_refactor.txt)
void launch_mac(const DevLevel *lv, int nlimbs, const MacJob *jobs, size_t n, int njobs, hipStream_t st, bool kara, bool packed, MacGrid grid)
{
    if (!njobs || !nlimbs) return;
    // (round 4, measured and not adopted -- tools/microbench/mac_persist.hip, profiles/r04_mac_{units,persist,stagger}.txt: a launch
    //  costs ~0.26 ms more than its chains' length explains, i.e. ~14 us per workgroup; long-lived workgroups that keep the load
    //  pipeline running across chains were 4-9 % SLOWER, starting the first resident generation in phases changed nothing)
    const unsigned gl = (unsigned)nlimbs, gj = (unsigned)njobs; const int ls = grid.limb_slow;
    const dim3 g = ls ? dim3(grid.gx, gj, gl) : dim3(grid.gx, gl, gj);
    if (packed) {
        if (kara) hipLaunchKernelGGL((k_mac<true, true>), g, dim3(EW_T), 0, st, lv, jobs, n, ls);
        else hipLaunchKernelGGL((k_mac<false, true>), g, dim3(EW_T), 0, st, lv, jobs, n, ls);
    } else if (kara) hipLaunchKernelGGL((k_mac<true, false>), g, dim3(EW_T), 0, st, lv, jobs, n, ls);
    else hipLaunchKernelGGL((k_mac<false, false>), g, dim3(EW_T), 0, st, lv, jobs, n, ls);
    KERNEL_CHECK();
}

// ---- single dyadic products on ONE limb (round 4): out[p][k] = a[k] * C_p[k] mod q_limb for p = 0, 1.
// The i = 0 block of eval_patstock (bin_bundle.cpp:314-324) switches every term a_j (.) C^j to the next level on its own, so
// the dropped limb of every term is needed by itself (k_i0_finish): terms x BinBundles chains of length ONE.  As k_mac jobs each
// of them paid a whole workgroup's fixed costs (descriptor and pointer reads, the first term's latency, the 128-bit fold, the
// drain of the stores: ~10 us at two workgroups per CU) for 1.4 us of work -- 9 % of the launch for 2.6 % of its bytes at
// 16M-4096, more at 256M-4096 (31 620 such chains).  Here: one thread per coefficient pair, ~40 registers, full occupancy.
template <bool PACKED>
__global__ __launch_bounds__(EW_T) void k_term_product(const DevLevel *__restrict__ lv, const TermJob *__restrict__ jobs, size_t njobs, size_t n, int limb,
                                                       u32 pw_poly_stride, u32 out_poly_stride)
{
    term_product_lane<PACKED>(lv, jobs, njobs, n, limb, pw_poly_stride, out_poly_stride, ((size_t)blockIdx.x * EW_T + threadIdx.x) * 2,
                              blockIdx.y + (size_t)gridDim.y * blockIdx.z);
}

void launch_term_product(const DevLevel *lv, const TermJob *jobs, size_t njobs, size_t n, int limb, u32 pw_poly_stride, u32 out_poly_stride,
                         bool packed, hipStream_t st)
{
    if (!njobs) return;
    const unsigned gy = (unsigned)std::min<size_t>(njobs, 32768), gz = (unsigned)((njobs + gy - 1) / gy);
    const dim3 grid((unsigned)((n / 2 + EW_T - 1) / EW_T), gy, gz);
    if (packed) hipLaunchKernelGGL((k_term_product<true>), grid, dim3(EW_T), 0, st, lv, jobs, njobs, n, limb, pw_poly_stride, out_poly_stride);
    else hipLaunchKernelGGL((k_term_product<false>), grid, dim3(EW_T), 0, st, lv, jobs, njobs, n, limb, pw_poly_stride, out_poly_stride);
    KERNEL_CHECK();
}

// ---- bit-packed database rows: dense u64 limbs <-> rows of mac_bits[j] bits per coefficient (DevLevel)
__global__ __launch_bounds__(EW_T) void k_pack_rows(const DevLevel *__restrict__ lv, int L, const u64 *__restrict__ dense, char *__restrict__ packed,
                                                    size_t slot_bytes, size_t n)
{
    pack_rows_lane(lv, L, dense, packed, slot_bytes, n, (size_t)blockIdx.x * EW_T + threadIdx.x, blockIdx.y / L, (int)(blockIdx.y % L));
}
__global__ __launch_bounds__(EW_T) void k_unpack_rows(const DevLevel *__restrict__ lv, int L, const char *__restrict__ packed, size_t slot_bytes,
                                                      u64 *__restrict__ dense, size_t n)
{
    unpack_rows_lane(lv, L, packed, slot_bytes, dense, n, (size_t)blockIdx.x * EW_T + threadIdx.x, blockIdx.y / L, (int)(blockIdx.y % L));
}
void launch_pack_rows(const DevLevel *lv, int L, const u64 *dense, void *packed, size_t slot_bytes, size_t n, size_t slots, hipStream_t st)
{
    if (!slots) return;
    hipLaunchKernelGGL(k_pack_rows, dim3((unsigned)((n * 2 + EW_T - 1) / EW_T), (unsigned)(slots * L)), dim3(EW_T), 0, st, lv, L, dense,
                       static_cast<char *>(packed), slot_bytes, n);
    KERNEL_CHECK();
}
void launch_unpack_rows(const DevLevel *lv, int L, const void *packed, size_t slot_bytes, u64 *dense, size_t n, size_t slots, hipStream_t st)
{
    if (!slots) return;
    hipLaunchKernelGGL(k_unpack_rows, dim3((unsigned)((n + EW_T - 1) / EW_T), (unsigned)(slots * L)), dim3(EW_T), 0, st, lv, L,
                       static_cast<const char *>(packed), slot_bytes, dense, n);
    KERNEL_CHECK();
}

} // namespace apsu_he
