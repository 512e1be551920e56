// Cuckoo hashing on the device, a translation unit of its own: every item's locations (the database side hashes each item under every
// function), the querier's table by the engine's order-independent rule, and the table's slot values.  Rules and contracts: cuckoo.h,
// which the CPU tier runs as well; launch_cuckoo.h.
#include "launch_cuckoo.h"
#include "kernel_launch.h"

#include <stdexcept>

namespace apsu_he {

// One lane per item, one 16-byte load, per staged group of G functions 16 LDS reads of G words, and one modulo per function.
// The bank of a read follows a random byte of the item whatever the layout, so a lane group spreads over the banks like balls over
// bins.  With one table per function (tab[f][pos][byte], ds_read_b32: 32 lanes on 32 banks, about 3.5 on the fullest) the LDS array
// took longer than the memory traffic (16 B in, 4 H B out per item): 16 H reads per item.  Interleaved (cuckoo_hash_group:
// img[pos][byte][G]) one ds_read_b128 serves four functions, 16 lanes on 16 slots of 16 bytes: a quarter of the reads, each of about
// the same cost.  H = 3 stages a fourth, empty column.  profiles/r24_cuckoo.txt has both.  The sixteen reads in flight
// take 81 registers a lane at G = 4, so one workgroup runs per compute unit (bounded to 64 registers the compiler spills).
template <int G>
__global__ __launch_bounds__(CUCKOO_LOC_T) void k_cuckoo_locations(const uint4 *__restrict__ items, size_t count, const u32 *__restrict__ tabs, u32 H,
                                                                   u32 T, u32 *__restrict__ locs)
{
    __shared__ __attribute__((aligned(16))) u32 lds[G * CUCKOO_TAB_WORDS];
    const u32 tid = threadIdx.x;
    for (u32 g0 = 0; g0 < H; g0 += G) {                              // workgroup-uniform
        const u32 ng = min((u32)G, H - g0);
        if (g0) __syncthreads();
        for (u32 idx = tid; idx < G * CUCKOO_TAB_WORDS; idx += CUCKOO_LOC_T)
            lds[cuckoo_group_image(idx, G)] = idx < ng * CUCKOO_TAB_WORDS ? tabs[(size_t)g0 * CUCKOO_TAB_WORDS + idx] : 0;
        __syncthreads();
        for (size_t i = (size_t)blockIdx.x * CUCKOO_LOC_T + tid; i < count; i += (size_t)gridDim.x * CUCKOO_LOC_T) {
            const uint4 it = items[i];
            u32 x[G];
            cuckoo_hash_group<G>(lds, it.x, it.y, it.z, it.w, x);
#pragma unroll
            for (u32 g = 0; g < (u32)G; g++)
                if (g < ng) locs[i * H + g0 + g] = x[g] % T;
        }
    }
}

void launch_cuckoo_locations(const unsigned char *items, size_t count, const u32 *tabs, u32 H, u32 T, u32 *locs, u32 wgs, hipStream_t st)
{
    if (!count) return;
    if (!H || H > CUCKOO_MAX_FUNCS || !T || ((uintptr_t)items & 15)) throw std::logic_error("launch_cuckoo_locations: outside its contract");
    if (!wgs) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
        wgs = 2 * (u32)cus;
    }
    const size_t need = (count + CUCKOO_LOC_T - 1) / CUCKOO_LOC_T;
    const dim3 grid((unsigned)std::min<size_t>(need, wgs));
    const uint4 *it = reinterpret_cast<const uint4 *>(items);
    static_assert(cuckoo_group(CUCKOO_MAX_FUNCS) == CUCKOO_LOC_GROUP, "the largest staged group");
    switch (cuckoo_group(H)) {
    case 1: hipLaunchKernelGGL(k_cuckoo_locations<1>, grid, dim3(CUCKOO_LOC_T), 0, st, it, count, tabs, H, T, locs); break;
    case 2: hipLaunchKernelGGL(k_cuckoo_locations<2>, grid, dim3(CUCKOO_LOC_T), 0, st, it, count, tabs, H, T, locs); break;
    default: hipLaunchKernelGGL(k_cuckoo_locations<4>, grid, dim3(CUCKOO_LOC_T), 0, st, it, count, tabs, H, T, locs); break;
    }
    KERNEL_CHECK();
}

// ---- the table.  One workgroup; item i belongs to lane i % CUCKOO_INSERT_T, which alone reads and writes state[i] and prop_round[i]
// (state: CuckooState | h_i << 2).  The slots take vector atomics only (ds_min_u64 / global_atomic_umin_x2); a slot in device memory
// is read back with an atomic load, which goes where the atomics went and not to a line the compute unit may still hold.
template <bool LDS_TABLE> __device__ __forceinline__ u64 cuckoo_slot_read(const u64 *p)
{
    if constexpr (LDS_TABLE) return *p;
    else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool LDS_TABLE>
__global__ __launch_bounds__(CUCKOO_INSERT_T) void k_cuckoo_insert(const unsigned char *__restrict__ items, const u32 *__restrict__ locs, u32 count,
                                                                   u32 H, u32 T, u64 max_rounds, u64 *gtable, u32 *state, u32 *prop_round,
                                                                   u32 *__restrict__ table_idx, u32 *__restrict__ item_loc, u64 *status)
{
    __shared__ u64 lds_table[LDS_TABLE ? CUCKOO_LDS_SLOTS : 1];
    __shared__ u32 any[2];                                           // round r votes in any[r & 1]: "some item is active again"
    u64 *table = LDS_TABLE ? lds_table : gtable;
    const u32 tid = threadIdx.x;
    for (u32 s = tid; s < T; s += CUCKOO_INSERT_T) table[s] = CUCKOO_EMPTY;
    for (u32 i = tid; i < count; i += CUCKOO_INSERT_T) state[i] = CUCKOO_ACTIVE;
    if (tid < 2) any[tid] = 0;
    if (tid == 0) { status[1] = ~(u64)0; status[2] = 0; }
    __syncthreads();
    u64 r = 0;
    bool more = count != 0;
    while (more && r < max_rounds) {                                 // workgroup-uniform
        for (u32 i = tid; i < count; i += CUCKOO_INSERT_T) {         // propose
            const u32 s = state[i];
            if ((s & 3) != CUCKOO_ACTIVE) continue;
            atomicMin(reinterpret_cast<unsigned long long *>(table + locs[(size_t)i * H + (s >> 2)]), (unsigned long long)cuckoo_key(max_rounds, r, i));
            prop_round[i] = (u32)r;
        }
        __syncthreads();
        if (tid == 0) any[(r + 1) & 1] = 0;                          // (its readers, of round r - 1, are all past the barrier above)
        for (u32 i = tid; i < count; i += CUCKOO_INSERT_T) {         // settle
            const u32 s = state[i];
            if ((s & 3) == CUCKOO_DUPLICATE) continue;
            u32 h = s >> 2;
            const u64 own = cuckoo_key(max_rounds, prop_round[i], i);
            const u64 v = cuckoo_slot_read<LDS_TABLE>(table + locs[(size_t)i * H + h]);
            const bool eq = v != own && cuckoo_items_equal(items + (size_t)cuckoo_key_item(v) * 16, items + (size_t)i * 16);
            const u32 ns = cuckoo_settle(own, v, eq);
            if (ns == CUCKOO_ACTIVE) { h = h + 1 == H ? 0 : h + 1; any[r & 1] = 1; }
            state[i] = ns | (h << 2);
        }
        __syncthreads();
        more = any[r & 1] != 0;
        r++;
    }
    for (u32 s = tid; s < T; s += CUCKOO_INSERT_T) {
        const u64 v = cuckoo_slot_read<LDS_TABLE>(table + s);
        table_idx[s] = v == CUCKOO_EMPTY ? CUCKOO_NONE : cuckoo_key_item(v);
    }
    u32 placed = 0;
    for (u32 i = tid; i < count; i += CUCKOO_INSERT_T) {
        const u32 s = state[i];
        item_loc[i] = (s & 3) == CUCKOO_DUPLICATE ? CUCKOO_NONE : locs[(size_t)i * H + (s >> 2)];
        if ((s & 3) == CUCKOO_ACTIVE) atomicMin(reinterpret_cast<unsigned long long *>(status + 1), (unsigned long long)i);
        placed += (s & 3) == CUCKOO_PLACED;
    }
    if (placed) atomicAdd(reinterpret_cast<unsigned long long *>(status + 2), (unsigned long long)placed);
    if (tid == 0) status[0] = r;
}

void launch_cuckoo_insert(bool lds_table, const unsigned char *items, const u32 *locs, u32 count, u32 H, u32 T, u64 max_rounds, u64 *table,
                          u32 *state, u32 *prop_round, u32 *table_idx, u32 *item_loc, u64 *status, hipStream_t st)
{
    if (!H || !T || !max_rounds || max_rounds > CUCKOO_MAX_ROUNDS || count >= CUCKOO_NONE) throw std::logic_error("launch_cuckoo_insert: outside its contract");
    if (lds_table) {
        if (T > CUCKOO_LDS_SLOTS) throw std::logic_error("the cuckoo table does not fit LDS: " + std::to_string(T) + " slots, " + std::to_string(CUCKOO_LDS_SLOTS) + " fit");
        hipLaunchKernelGGL(k_cuckoo_insert<true>, dim3(1), dim3(CUCKOO_INSERT_T), 0, st, items, locs, count, H, T, max_rounds, table, state, prop_round,
                           table_idx, item_loc, status);
    } else {
        hipLaunchKernelGGL(k_cuckoo_insert<false>, dim3(1), dim3(CUCKOO_INSERT_T), 0, st, items, locs, count, H, T, max_rounds, table, state, prop_round,
                           table_idx, item_loc, status);
    }
    KERNEL_CHECK();
}

// one lane per slot value; the F lanes of an item read the same 16 bytes
__global__ __launch_bounds__(EW_T) void k_query_values(const u64 *__restrict__ table_items, u32 items_per_bundle, u32 F, u32 bpf, u32 item_bits, size_t n,
                                                       u64 *__restrict__ values)
{
    const size_t p = (size_t)blockIdx.x * EW_T + threadIdx.x;
    if (p >= n) return;
    const u32 b = blockIdx.y;
    u32 j = 0;
    const u32 slot = query_value_slot(b, (u32)p, items_per_bundle, F, &j);
    u64 v = 0;
    if (slot != CUCKOO_NONE) v = cuckoo_item_felt(table_items[(size_t)slot * 2], table_items[(size_t)slot * 2 + 1], j, bpf, item_bits);
    values[(size_t)b * n + p] = v;
}

void launch_query_values(const unsigned char *table_items, u32 nb, u32 items_per_bundle, u32 F, u32 bpf, u32 item_bits, size_t n, u64 *values,
                         hipStream_t st)
{
    if (!nb) return;
    if (!F || (size_t)items_per_bundle * F > n || nb > 65535 || ((uintptr_t)table_items & 7)) throw std::logic_error("launch_query_values: outside its contract");
    hipLaunchKernelGGL(k_query_values, ew_grid(n, (int)nb), dim3(EW_T), 0, st, reinterpret_cast<const u64 *>(table_items), items_per_bundle, F, bpf,
                       item_bits, n, values);
    KERNEL_CHECK();
}

} // namespace apsu_he
