// The placement rule of the database-level step (Engine::apply_entries), as pure functions of what the lookup found: which BinBundle
// of one bundle index an entry is removed from or inserted into, and when a new BinBundle is appended.  No HIP in here; the CPU tier
// reaches it through the emulation library (emu/db.cpp: emu_place_entries, tests/test_bundle_lookup_cpu.py).
//
// It restates ReceiverDB::remove's and ReceiverDB::insert_or_assign's loops (receiver_db.cpp:349-434,524-567) over counts and
// root tests instead of the host-side item lists the reference keeps:
//   * removals come first (as in apsu_he_bundle_update): an entry leaves the FIRST BinBundle in cache order that holds it (:543-549);
//     one that no BinBundle holds is NOT_FOUND and changes nothing.  A BinBundle all of whose bins are empty after the removals is
//     EMPTY: the caller drops it (:551-555), and like the reference's erased BinBundle it takes no insertion of this call.
//   * insertions follow in list order.  An entry that some BinBundle holds, or that equals an entry placed earlier in the same call, is
//     a DUPLICATE (the role of hashed_items_, :988-1000).  Otherwise the BinBundles are tried newest first (:370); the entry fits iff
//     every slot s + j is a bin and max_j(count[s + j] + 1) < max_items_per_bin -- strictly (:388-389) -- with the counts as the
//     entries before it (and this call's removals) have left them.  If it fits nowhere a new BinBundle is appended, takes the entry
//     unconditionally (:410-433) and is the newest from then on.
// "Holds" is the root test of every part in its own bin (bin_lookup.h), taken BEFORE this call changes anything.  It includes the
// reference's false positive -- every part present in its bin, each from a different item -- and it cannot tell how often a value is
// in a bin: two removals that name the same value of the same bin are both scheduled, and the division in k_bins_update is the judge.
#pragma once
#include <algorithm>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "bin_lookup.h"

namespace apsu_he {

enum PlaceStatus : u32 { PLACE_INSERTED = 0, PLACE_DUPLICATE = 1, PLACE_REMOVED = 2, PLACE_NOT_FOUND = 3 };
enum PlaceState : u32 { PLACE_UNCHANGED = 0, PLACE_REPLACED = 1, PLACE_EMPTY = 2 };
constexpr u32 PLACE_NO_TARGET = 0xFFFFFFFFu;

struct PlaceLists {                                       // apsu_he_bundle_update's layout: roots[bin * stride + r], r < counts[bin]
    u32 stride = 0;
    std::vector<u64> roots;
    std::vector<u32> counts;
    bool any() const { return stride != 0; }
};

struct PlaceInput {
    u32 n_bundles = 0, bins = 0, F = 0, max_items = 0;
    u64 t = 0;
    const u32 *counts = nullptr;                          // [n_bundles][bins], cache order; LOOKUP_NONE: the slot is not a bin
    const unsigned char *ins_present = nullptr;           // [n_bundles][n_ins]
    const unsigned char *rem_present = nullptr;           // [n_bundles][n_rem]
    const u64 *ins_felts = nullptr, *rem_felts = nullptr; // [count][F]
    const u32 *ins_start = nullptr, *rem_start = nullptr;
    size_t n_ins = 0, n_rem = 0;
};

struct PlaceResult {
    std::vector<u32> ins_status, ins_target, rem_status, rem_target;   // target: position among the given BinBundles, then the appended ones
    std::vector<u32> state;                               // per given BinBundle
    u32 n_new = 0;
    std::vector<PlaceLists> ins, rem;                     // [n_bundles + n_new]; rem is empty for the appended ones
};

// every refusal of the call, before anything is decided: std::invalid_argument
inline void place_validate(const u64 *ins_felts, const u32 *ins_start, size_t n_ins, const u64 *rem_felts, const u32 *rem_start, size_t n_rem,
                           u32 F, u32 bins, u64 t)
{
    if (!F) throw std::invalid_argument("felts_per_item is 0");
    std::map<std::vector<u64>, int> seen;                 // entry -> 1: in the removal list
    for (int list = 0; list < 2; list++) {
        const u64 *felts = list ? ins_felts : rem_felts;
        const u32 *start = list ? ins_start : rem_start;
        const size_t count = list ? n_ins : n_rem;
        for (size_t e = 0; e < count; e++) {
            const std::string what = std::string(list ? "insert" : "remove") + " entry " + std::to_string(e);
            if ((u64)start[e] + F > bins) throw std::invalid_argument(what + ": start bin + felts_per_item exceeds bins_per_bundle");
            std::vector<u64> key{ start[e] };
            for (u32 j = 0; j < F; j++) {
                if (felts[e * F + j] >= t) throw std::invalid_argument(what + ": field element is not reduced modulo plain_modulus");
                key.push_back(felts[e * F + j]);
            }
            if (!list) {
                if (!seen.emplace(std::move(key), 1).second) throw std::invalid_argument(what + " appears twice in the removal list");
            } else if (seen.count(key)) throw std::invalid_argument(what + " is in the removal list too");
        }
    }
}

inline PlaceLists place_flatten(const std::vector<std::vector<u64>> &per_bin)
{
    PlaceLists out;
    size_t stride = 0;
    for (const auto &b : per_bin) stride = std::max(stride, b.size());
    if (!stride) return out;
    out.stride = (u32)stride;
    out.roots.assign(per_bin.size() * stride, 0);
    out.counts.assign(per_bin.size(), 0);
    for (size_t s = 0; s < per_bin.size(); s++) {
        out.counts[s] = (u32)per_bin[s].size();
        std::copy(per_bin[s].begin(), per_bin[s].end(), out.roots.begin() + s * stride);
    }
    return out;
}

inline PlaceResult place_entries(const PlaceInput &in)
{
    place_validate(in.ins_felts, in.ins_start, in.n_ins, in.rem_felts, in.rem_start, in.n_rem, in.F, in.bins, in.t);
    const u32 nb = in.n_bundles, bins = in.bins, F = in.F;
    PlaceResult out;
    out.ins_status.assign(in.n_ins, PLACE_DUPLICATE);
    out.ins_target.assign(in.n_ins, PLACE_NO_TARGET);
    out.rem_status.assign(in.n_rem, PLACE_NOT_FOUND);
    out.rem_target.assign(in.n_rem, PLACE_NO_TARGET);
    out.state.assign(nb, PLACE_UNCHANGED);
    std::vector<std::vector<u32>> cnt(nb);
    for (u32 b = 0; b < nb; b++) cnt[b].assign(in.counts + (size_t)b * bins, in.counts + (size_t)(b + 1) * bins);
    std::vector<std::vector<std::vector<u64>>> ins(nb, std::vector<std::vector<u64>>(bins)), rem(nb, std::vector<std::vector<u64>>(bins));

    for (size_t e = 0; e < in.n_rem; e++)
        for (u32 b = 0; b < nb; b++) {
            if (!in.rem_present[(size_t)b * in.n_rem + e]) continue;
            const u32 s = in.rem_start[e];
            for (u32 j = 0; j < F; j++) {
                // (a count is only consumed once per scheduled removal; when two removals share a value whose bin holds it once, the
                //  count may reach 0 here and the update's division refuses the second)
                if (cnt[b][s + j] != LOOKUP_NONE && cnt[b][s + j] > 0) cnt[b][s + j]--;
                rem[b][s + j].push_back(in.rem_felts[e * F + j]);
            }
            out.rem_status[e] = PLACE_REMOVED;
            out.rem_target[e] = b;
            out.state[b] = PLACE_REPLACED;
            break;
        }
    for (u32 b = 0; b < nb; b++) {
        bool empty = true;
        for (u32 s = 0; s < bins && empty; s++) empty = cnt[b][s] == LOOKUP_NONE || cnt[b][s] == 0;
        if (empty) out.state[b] = PLACE_EMPTY;
    }

    std::map<std::vector<u64>, u32> placed;               // entries placed by this call -> target
    for (size_t e = 0; e < in.n_ins; e++) {
        const u32 s = in.ins_start[e];
        const u64 *f = in.ins_felts + e * F;
        bool dup = false;
        for (u32 b = 0; b < nb && !dup; b++)
            if (in.ins_present[(size_t)b * in.n_ins + e]) { dup = true; out.ins_target[e] = b; }
        std::vector<u64> key{ s };
        key.insert(key.end(), f, f + F);
        if (!dup) {
            auto it = placed.find(key);
            if (it != placed.end()) { dup = true; out.ins_target[e] = it->second; }
        }
        if (dup) continue;                                // status stays PLACE_DUPLICATE
        u32 target = PLACE_NO_TARGET;
        for (u32 b = (u32)cnt.size(); b-- > 0 && target == PLACE_NO_TARGET;) {          // newest first
            if (b < nb && out.state[b] == PLACE_EMPTY) continue;
            u32 room = 0;
            for (u32 j = 0; j < F && room != LOOKUP_NONE; j++) room = cnt[b][s + j] == LOOKUP_NONE ? LOOKUP_NONE : std::max(room, cnt[b][s + j] + 1);
            if (room != LOOKUP_NONE && room < in.max_items) target = b;
        }
        if (target == PLACE_NO_TARGET) {                  // a fresh BinBundle: every bin holds the polynomial 1
            target = (u32)cnt.size();
            cnt.emplace_back(bins, 0);
            ins.emplace_back(bins);
        }
        for (u32 j = 0; j < F; j++) {
            cnt[target][s + j]++;
            ins[target][s + j].push_back(f[j]);
        }
        if (target < nb) out.state[target] = PLACE_REPLACED;
        out.ins_status[e] = PLACE_INSERTED;
        out.ins_target[e] = target;
        placed.emplace(std::move(key), target);
    }
    out.n_new = (u32)cnt.size() - nb;
    for (size_t b = 0; b < cnt.size(); b++) {
        out.ins.push_back(place_flatten(ins[b]));
        out.rem.push_back(b < nb ? place_flatten(rem[b]) : PlaceLists());
    }
    return out;
}

}  // namespace apsu_he
