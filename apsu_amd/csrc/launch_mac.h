// Launch entry points of the multiply-accumulate family (kernels_mac.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "dev_consts.h"
#include "mac_plan.h"

namespace apsu_he {

// k_mac over njobs MacJobs (mac_core.h) in the form (kara: three products; packed: bit-packed plaintexts) and on the grid of a MacPlan (mac_plan.h)
void launch_mac(const DevLevel *lv, int nlimbs, const MacJob *jobs, size_t n, int njobs, hipStream_t st, bool kara, bool packed, MacGrid grid);
// single products on one limb: out[0][k] = a[k] * pw[limb][k], out[out_poly_stride + k] = a[k] * pw[pw_poly_stride + limb n + k]  (mod q_limb);
// pt: the plaintext's slot as k_mac takes it (dense: [L][n] words; packed: the bit-packed slot, rows per DevLevel::mac_row_off)
void launch_term_product(const DevLevel *lv, const TermJob *jobs, size_t njobs, size_t n, int limb, u32 pw_poly_stride, u32 out_poly_stride,
                         bool packed, hipStream_t st);
// dense [slots][L][n] u64 <-> bit-packed [slots][slot_bytes] (rows per DevLevel::mac_bits / mac_row_off of `lv`)
void launch_pack_rows(const DevLevel *lv, int L, const u64 *dense, void *packed, size_t slot_bytes, size_t n, size_t slots, hipStream_t st);
void launch_unpack_rows(const DevLevel *lv, int L, const void *packed, size_t slot_bytes, u64 *dense, size_t n, size_t slots, hipStream_t st);

} // namespace apsu_he
