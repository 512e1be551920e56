// CPU emulation of building a whole database from its entries (bulk_place.h): the closed-form placement rule and the lane body of
// k_entries_scatter stepped over every lane of its grid.  A library of its own, libapsu_he_hostemu_bulk.so, next to
// libapsu_he_hostemu.so: that library's set of exports is pinned by tests/test_emu_lib_cpu.py, which holds the loader's table of return
// types to it.  Only tests load it (tests/test_bulk_place_cpu.py); like the other emulation units it is not a fallback path.
#include <algorithm>
#include <stdexcept>
#include <vector>

#include "../emu/emu_common.h"
#include "bulk_place.h"

using namespace apsu_he;

extern "C" {

const char *emu_bulk_last_error() { return g_err.c_str(); }   // the text of the calling thread's last refusal in this library

// ---- a whole database from its entries (bulk_place.h)
// bulk_plan: kstart [T], bundles [T / items_per_bundle], *total.  Returns 0, or -1 for a refusal (std::invalid_argument; emu_bulk_last_error).
int emu_bulk_plan(const uint64_t *offsets, uint64_t T, uint32_t items_per_bundle, uint32_t max_items_per_bin, uint32_t *kstart, uint32_t *bundles, uint64_t *total)
{
    try {
        const BulkPlan p = bulk_plan(offsets, T, items_per_bundle, max_items_per_bin);
        std::copy(p.kstart.begin(), p.kstart.end(), kstart);
        std::copy(p.bundles.begin(), p.bundles.end(), bundles);
        *total = p.total;
        return 0;
    } catch (const std::invalid_argument &e) { g_err = e.what(); return -1;
    } catch (const std::exception &e) { g_err = e.what(); return -3; }
}

// k_entries_scatter for target BinBundle k of one bundle index as its grid runs it: entries_scatter_lane stepped over every lane of
// (locations + 1) x blocks workgroups (blocks 0: scatter_blocks' choice).  items [offsets[locations] - offsets[0]][2] words; roots
// [bins][stride] and counts [n_counts] come in holding what the words nobody writes keep.  Returns the workgroups per location, or -1
// (emu_bulk_last_error) for what launch_entries_scatter refuses, a chunk longer than `stride`, or bins below locations * F.
int emu_entries_scatter(const uint64_t *items, const uint64_t *offsets, const uint32_t *kstart, uint32_t locations, uint32_t F, uint32_t bpf,
                        uint32_t item_bits, uint32_t cap, uint32_t k, uint32_t stride, uint32_t bins, uint64_t *roots, uint32_t *counts, uint32_t n_counts,
                        uint32_t blocks)
{
    return guarded([&]() -> int {
        if (!F || F > SCATTER_MAX_F || !bpf || bpf > 64 || (u64)(F - 1) * bpf >= 128) throw std::invalid_argument("felts_per_item or bits per felt out of range");
        if (!cap || !stride || stride >= ((u32)1 << 30)) throw std::invalid_argument("cap or stride out of range");
        if ((u64)locations * F > n_counts || (u64)locations * F > bins) throw std::invalid_argument("more bins than count words or root lists");
        for (u32 l = 0; l < locations; l++) {
            if (offsets[l + 1] < offsets[l] || offsets[l + 1] - offsets[l] > 0xFFFFFFFFull) throw std::invalid_argument("offsets decrease, or a location holds more than 2^32 - 1 entries");
            if (bulk_chunk(kstart[l], (u32)(offsets[l + 1] - offsets[l]), k, cap).len > stride) throw std::invalid_argument("a chunk is longer than stride");
        }
        if (!blocks) blocks = scatter_blocks(locations, cap);
        std::vector<BulkItem> it(offsets[locations] - offsets[0]);     // (16-byte aligned, as the kernel's loads want them)
        for (size_t i = 0; i < it.size(); i++) it[i] = BulkItem{ items[2 * i], items[2 * i + 1] };
        for (u32 loc = 0; loc <= locations; loc++)
            for (u32 by = 0; by < blocks; by++)
                for (u32 tid = 0; tid < (u32)SCATTER_T; tid++)
                    entries_scatter_lane(it.data(), offsets, kstart, locations, F, bpf, item_bits, cap, k, stride, roots, counts, n_counts, loc, by, blocks, tid, SCATTER_T);
        return (int)blocks;
    });
}

} // extern "C"
