// See multi.h: the resident database maintained on the multi-device handle.  The counterpart, for a database spread over several
// devices, of ReceiverDB::insert_or_assign / remove (receiver_db.cpp:330-433,524-567) and of the single-context calls
// Engine::apply_entries / compact: the same kernels run on the device that owns a BinBundle, the host steps (place_entries,
// plan_compaction) are the single context's, and the rules that only a handle needs are multi_place.h's.
#include "multi.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace apsu_he {

struct MultiEngine::Change {
    std::vector<unsigned char> dropped;                           // [old count]
    std::vector<std::unique_ptr<Bundle>> replaced;                // [old count]: the BinBundle that takes the id's place, else null
    std::vector<std::pair<int, std::unique_ptr<Bundle>>> appended;   // (slot, BinBundle) in order of appending
    explicit Change(size_t count) : dropped(count, 0), replaced(count) {}
};

std::vector<RegUnit> MultiEngine::registry_locked() const
{
    std::vector<RegUnit> reg(where_.size());
    for (size_t i = 0; i < where_.size(); i++) {
        const Bundle &b = bundle_locked((int)i);
        reg[i].slot = where_[i].first; reg[i].bundle_idx = b.bundle_idx; reg[i].cache_idx = b.cache_idx; reg[i].degree = b.degree;
    }
    return reg;
}

void MultiEngine::check_id(int id) const
{
    if (id < 0 || (size_t)id >= where_.size()) throw std::invalid_argument("no BinBundle with this id");
}

// The one place where ids and rows change.  Everything that can fail comes first: the renumbering (registry_after), the wait for every
// engine that owns a BinBundle which is replaced or dropped, the allocations.  What is replaced or dropped is freed at the end.
void MultiEngine::commit(Change &c, int *new_id, std::vector<int> *new_id_out)
{
    const std::vector<RegUnit> old = registry_locked();
    std::vector<int64_t> replaced_degree(old.size(), -1);
    std::vector<RegUnit> app;
    for (size_t i = 0; i < old.size(); i++)
        if (c.replaced[i]) replaced_degree[i] = c.replaced[i]->degree;
    for (const auto &a : c.appended) {
        RegUnit u;
        u.slot = a.first; u.bundle_idx = a.second->bundle_idx; u.cache_idx = a.second->cache_idx; u.degree = a.second->degree;
        app.push_back(u);
    }
    const RegistryAfter ra = registry_after(old, c.dropped, replaced_degree, app);
    std::vector<char> touched(devs_.size(), 0);
    for (size_t i = 0; i < old.size(); i++)
        if (c.dropped[i] || c.replaced[i]) touched[(size_t)old[i].slot] = 1;
    run_all([&](Dev &d) { if (touched[(size_t)d.slot]) d.eng->drain(); });   // evaluations with device-side results may still read the old rows
    const size_t count = ra.registry.size();
    std::vector<std::unique_ptr<Bundle>> next(count), gone;
    gone.reserve(old.size());
    std::vector<std::pair<int, int>> where(count);
    std::vector<std::vector<std::unique_ptr<Bundle>>> rows(devs_.size());
    std::vector<std::vector<int>> ids(devs_.size());
    std::vector<size_t> per_slot(devs_.size(), 0);
    for (const RegUnit &u : ra.registry) per_slot[(size_t)u.slot]++;
    for (size_t s = 0; s < devs_.size(); s++) { rows[s].reserve(per_slot[s]); ids[s].reserve(per_slot[s]); }
    std::vector<int> copy_out(ra.new_id);
    // ---- nothing throws from here on
    for (size_t i = 0; i < old.size(); i++) {
        std::unique_ptr<Bundle> &cur = devs_[(size_t)where_[i].first]->bundles[(size_t)where_[i].second];
        const int to = ra.new_id[i];
        if (to < 0) { gone.push_back(std::move(cur)); continue; }
        if (c.replaced[i]) { gone.push_back(std::move(cur)); next[(size_t)to] = std::move(c.replaced[i]); }
        else next[(size_t)to] = std::move(cur);
    }
    for (size_t k = 0; k < c.appended.size(); k++) next[(size_t)ra.new_id[old.size() + k]] = std::move(c.appended[k].second);
    for (size_t k = 0; k < count; k++) {
        const size_t s = (size_t)ra.registry[k].slot;
        where[k] = { (int)s, (int)rows[s].size() };
        rows[s].push_back(std::move(next[k]));
        ids[s].push_back((int)k);
    }
    for (size_t s = 0; s < devs_.size(); s++) { devs_[s]->bundles.swap(rows[s]); devs_[s]->ids.swap(ids[s]); }
    where_.swap(where);
    if (new_id) std::copy(copy_out.begin(), copy_out.end(), new_id);
    if (new_id_out) new_id_out->swap(copy_out);
}

std::vector<RegUnit> MultiEngine::registry()
{
    std::lock_guard<std::mutex> g(mu_);
    return registry_locked();
}

std::vector<int> MultiEngine::index_bundles(uint32_t bundle_idx)
{
    std::lock_guard<std::mutex> g(mu_);
    if (bundle_idx >= psu_.bundle_idx_count) throw std::invalid_argument("bundle_idx out of range");
    return index_in_cache_order(registry_locked(), bundle_idx);
}

void MultiEngine::export_saved_db(const std::string &path, const wire::ReceiverDbHeaderParts &header, const uint64_t ntt_parms_id[4], uint32_t flags, int compr)
{
    std::lock_guard<std::mutex> g(mu_);
    std::vector<Engine *> engs;
    std::vector<const Bundle *> bs;
    const std::vector<RegUnit> reg = registry_locked();
    for (uint32_t idx = 0; idx < psu_.bundle_idx_count; idx++)
        for (int id : index_in_cache_order(reg, idx)) {
            engs.push_back(devs_[(size_t)where_[(size_t)id].first]->eng.get());
            bs.push_back(&bundle_locked(id));
        }
    saved_db_export(path, engs.data(), bs.data(), bs.size(), header, ntt_parms_id, flags, compr);
}

void MultiEngine::bin_counts(int id, uint32_t *counts)
{
    std::lock_guard<std::mutex> g(mu_);
    check_id(id);
    devs_[(size_t)where_[(size_t)id].first]->eng->bin_counts(bundle_locked(id), counts);
}

void MultiEngine::bundle_bins(int id, u64 *roots, uint32_t *counts, uint32_t stride)
{
    std::lock_guard<std::mutex> g(mu_);
    check_id(id);
    devs_[(size_t)where_[(size_t)id].first]->eng->bundle_bins(bundle_locked(id), roots, counts, stride);
}

// Every device tests the BinBundles it owns, devices side by side, each with the query of the WHOLE database's bundle indices and the
// mask draws of its BinBundles' ids: what one context holding all of them would draw.  Positions become ids before the reports are reduced.
SelfTestReport MultiEngine::self_test(const u64 seed[8])
{
    std::lock_guard<std::mutex> g(mu_);
    std::vector<uint32_t> idx;
    for (const RegUnit &u : registry_locked()) idx.push_back(u.bundle_idx);
    std::sort(idx.begin(), idx.end());
    idx.erase(std::unique(idx.begin(), idx.end()), idx.end());
    std::vector<SelfTestReport> parts(devs_.size(), self_test_empty());
    run_all([&](Dev &d) {
        std::vector<size_t> order(d.bundles.size());                  // by id: a part's first mismatch is then its lowest id's
        for (size_t i = 0; i < order.size(); i++) order[i] = i;
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return d.ids[a] < d.ids[b]; });
        std::vector<const Bundle *> bs;
        std::vector<uint32_t> ids;
        for (size_t i : order) { bs.push_back(d.bundles[i].get()); ids.push_back((uint32_t)d.ids[i]); }
        // (a device that owns nothing still answers for its context: the refusals are every device's)
        SelfTestReport r = d.eng->self_test(bs.data(), (uint32_t)bs.size(), seed, nullptr, idx.data(), (uint32_t)idx.size(), ids.data());
        if (r.first_bundle >= 0) r.first_bundle = (int32_t)ids[(size_t)r.first_bundle];
        if (r.min_budget_bundle >= 0) r.min_budget_bundle = (int32_t)ids[(size_t)r.min_budget_bundle];
        parts[(size_t)d.slot] = r;
    });
    SelfTestReport rep = self_test_empty();
    for (const SelfTestReport &r : parts) self_test_reduce(rep, r);
    return rep;
}

int MultiEngine::build_bundle(int slot, uint32_t bundle_idx, uint32_t cache_idx, const u64 *roots, const uint32_t *counts, uint32_t bins, uint32_t stride)
{
    std::lock_guard<std::mutex> g(mu_);
    if (slot == -1) {
        const std::vector<uint64_t> load = device_loads(registry_locked(), (int)devs_.size());
        slot = place_new_unit(bundle_idx, psu_.bundle_idx_count, (int)devs_.size(), load.data());
    }
    if (slot < 0 || slot >= (int)devs_.size()) throw std::invalid_argument("device slot out of range");
    Dev &d = *devs_[(size_t)slot];
    std::unique_ptr<Bundle> b = d.eng->build_bundle(bundle_idx, cache_idx, roots, counts, bins, stride);
    d.bundles.reserve(d.bundles.size() + 1); d.ids.reserve(d.ids.size() + 1); where_.reserve(where_.size() + 1);
    const int id = (int)where_.size();
    d.bundles.push_back(std::move(b));
    d.ids.push_back(id);
    where_.push_back({ slot, (int)d.bundles.size() - 1 });
    return id;
}

void MultiEngine::remove_bundle(int id, int *new_id)
{
    std::lock_guard<std::mutex> g(mu_);
    check_id(id);
    Change c(where_.size());
    c.dropped[(size_t)id] = 1;
    commit(c, new_id, nullptr);
}

void MultiEngine::move_bundle(int id, int slot)
{
    std::lock_guard<std::mutex> g(mu_);
    check_id(id);
    if (slot < 0 || slot >= (int)devs_.size()) throw std::invalid_argument("device slot out of range");
    const int from = where_[(size_t)id].first;
    if (from == slot) return;
    Dev &src = *devs_[(size_t)from], &dst = *devs_[(size_t)slot];
    std::unique_ptr<Bundle> moved = dst.eng->clone_bundle(bundle_locked(id), src.device);
    src.eng->drain();                                             // an evaluation with device-side results may still read the old rows
    dst.bundles.reserve(dst.bundles.size() + 1);
    dst.ids.reserve(dst.ids.size() + 1);
    // ---- nothing throws from here on
    const size_t at_src = (size_t)where_[(size_t)id].second;
    std::unique_ptr<Bundle> gone = std::move(src.bundles[at_src]);
    src.bundles.erase(src.bundles.begin() + (std::ptrdiff_t)at_src);
    src.ids.erase(src.ids.begin() + (std::ptrdiff_t)at_src);
    const size_t at_dst = (size_t)(std::lower_bound(dst.ids.begin(), dst.ids.end(), id) - dst.ids.begin());   // rows of a device stay in id order
    dst.bundles.insert(dst.bundles.begin() + (std::ptrdiff_t)at_dst, std::move(moved));
    dst.ids.insert(dst.ids.begin() + (std::ptrdiff_t)at_dst, id);
    for (Dev *d : { &src, &dst })
        for (size_t i = 0; i < d->ids.size(); i++) where_[(size_t)d->ids[i]] = { d->slot, (int)i };
}

void MultiEngine::lookup(uint32_t bundle_idx, const u64 *felts, const uint32_t *start, size_t count, unsigned char *present, uint32_t *room)
{
    std::lock_guard<std::mutex> g(mu_);
    if (bundle_idx >= psu_.bundle_idx_count) throw std::invalid_argument("bundle_idx out of range");
    const std::vector<RegUnit> reg = registry_locked();
    const std::vector<int> ids = index_in_cache_order(reg, bundle_idx);
    std::vector<std::vector<size_t>> mine(devs_.size());          // positions in cache order, per device
    for (size_t p = 0; p < ids.size(); p++) mine[(size_t)reg[(size_t)ids[p]].slot].push_back(p);
    run_all([&](Dev &d) {
        const std::vector<size_t> &pos = mine[(size_t)d.slot];
        if (pos.empty()) return;
        std::vector<const Bundle *> bs;
        for (size_t p : pos) bs.push_back(&bundle_locked(ids[p]));
        std::vector<unsigned char> lp(pos.size() * count);
        std::vector<uint32_t> lr(pos.size() * count);
        d.eng->lookup_bundles(bs.data(), (uint32_t)bs.size(), felts, start, count, lp.data(), lr.data());
        for (size_t i = 0; i < pos.size(); i++) {
            if (present) std::copy(lp.begin() + (std::ptrdiff_t)(i * count), lp.begin() + (std::ptrdiff_t)((i + 1) * count), present + pos[i] * count);
            if (room) std::copy(lr.begin() + (std::ptrdiff_t)(i * count), lr.begin() + (std::ptrdiff_t)((i + 1) * count), room + pos[i] * count);
        }
    });
}

MultiEngine::ApplyOutcome MultiEngine::apply_entries(uint32_t bundle_idx, const u64 *ins_felts, const uint32_t *ins_start, size_t n_ins,
                                                     const u64 *rem_felts, const uint32_t *rem_start, size_t n_rem)
{
    std::lock_guard<std::mutex> g(mu_);
    ApplyOutcome res;
    const size_t n = hp_.n;
    const uint32_t F = psu_.item_params.felts_per_item, bins = psu_.bins_per_bundle;
    devs_[0]->eng->lookup_counts("apply_entries", nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr);       // the context's own refusals
    if (bundle_idx >= psu_.bundle_idx_count) throw std::invalid_argument("bundle_idx out of range");
    const std::vector<RegUnit> reg = registry_locked();
    res.ids = index_in_cache_order(reg, bundle_idx);
    res.old_count = (int)reg.size();
    const std::vector<int> &ids = res.ids;
    const uint32_t nb = (uint32_t)ids.size();
    // the refusals come before any GPU work
    place_validate(ins_felts, ins_start, n_ins, rem_felts, rem_start, n_rem, F, bins, hp_.t);
    // 1. one lookup per device for both lists: removals first, insertions behind them
    const size_t count = n_rem + n_ins;
    std::vector<u64> felts(count * F);
    std::vector<uint32_t> start(count);
    std::copy(rem_felts, rem_felts + n_rem * F, felts.begin());
    std::copy(ins_felts, ins_felts + n_ins * F, felts.begin() + (std::ptrdiff_t)(n_rem * F));
    std::copy(rem_start, rem_start + n_rem, start.begin());
    std::copy(ins_start, ins_start + n_ins, start.begin() + (std::ptrdiff_t)n_rem);
    std::vector<std::vector<size_t>> mine(devs_.size());          // positions in cache order, per device
    for (size_t p = 0; p < nb; p++) mine[(size_t)reg[(size_t)ids[p]].slot].push_back(p);
    std::vector<uint32_t> counts((size_t)nb * n);
    std::vector<unsigned char> present((size_t)nb * count);
    run_all([&](Dev &d) {
        const std::vector<size_t> &pos = mine[(size_t)d.slot];
        if (pos.empty()) return;
        std::vector<const Bundle *> bs;
        for (size_t p : pos) bs.push_back(&bundle_locked(ids[p]));
        std::vector<uint32_t> lc(pos.size() * n);
        std::vector<unsigned char> lp(pos.size() * count);
        d.eng->lookup_counts("apply_entries", bs.data(), (uint32_t)bs.size(), felts.data(), start.data(), count, lc.data(), lp.data());
        for (size_t i = 0; i < pos.size(); i++) {
            std::copy(lc.begin() + (std::ptrdiff_t)(i * n), lc.begin() + (std::ptrdiff_t)((i + 1) * n), counts.begin() + (std::ptrdiff_t)(pos[i] * n));
            std::copy(lp.begin() + (std::ptrdiff_t)(i * count), lp.begin() + (std::ptrdiff_t)((i + 1) * count), present.begin() + (std::ptrdiff_t)(pos[i] * count));
        }
    });
    // 2. the placement, over the rows in cache order
    res.place = place_from_lookup(nb, n, bins, F, psu_.table_params.max_items_per_bin, hp_.t, counts.data(), present.data(), ins_felts, ins_start, n_ins,
                                  rem_felts, rem_start, n_rem);
    const PlaceResult &pl = res.place;
    // 3. every changed BinBundle is rebuilt on its device
    Change c(reg.size());
    run_all([&](Dev &d) {
        for (size_t p : mine[(size_t)d.slot]) {
            if (pl.state[p] != PLACE_REPLACED) continue;
            const PlaceLists &li = pl.ins[p], &lr = pl.rem[p];
            c.replaced[(size_t)ids[p]] = d.eng->update_bundle(bundle_locked(ids[p]), li.any() ? li.roots.data() : nullptr, li.any() ? li.counts.data() : nullptr,
                                                              li.stride, lr.any() ? lr.roots.data() : nullptr, lr.any() ? lr.counts.data() : nullptr, lr.stride, bins);
        }
    });
    // 4. the appended BinBundles: loads as the updates left them (an EMPTY BinBundle still counts, it leaves at the commit), placed in order
    std::vector<RegUnit> now = reg;
    for (size_t i = 0; i < now.size(); i++)
        if (c.replaced[i]) now[i].degree = c.replaced[i]->degree;
    std::vector<uint64_t> load = device_loads(now, (int)devs_.size());
    std::vector<int> app_slot(pl.n_new);
    for (uint32_t k = 0; k < pl.n_new; k++) {
        const PlaceLists &li = pl.ins[nb + k];
        const uint32_t degree = li.counts.empty() ? 0 : *std::max_element(li.counts.begin(), li.counts.end());   // build_bundle's
        app_slot[k] = place_new_unit(bundle_idx, psu_.bundle_idx_count, (int)devs_.size(), load.data());
        load[(size_t)app_slot[k]] += unit_cost(degree);
    }
    const uint32_t next_cache = nb ? reg[(size_t)ids[nb - 1]].cache_idx + 1 : 0;
    std::vector<std::unique_ptr<Bundle>> built(pl.n_new);
    run_all([&](Dev &d) {
        for (uint32_t k = 0; k < pl.n_new; k++) {
            if (app_slot[k] != d.slot) continue;
            const PlaceLists &li = pl.ins[nb + k];
            built[k] = d.eng->build_bundle(bundle_idx, next_cache + k, li.roots.data(), li.counts.data(), bins, li.stride);
        }
    });
    for (uint32_t k = 0; k < pl.n_new; k++) c.appended.push_back({ app_slot[k], std::move(built[k]) });
    // 5., 6. EMPTY BinBundles leave, everybody is renumbered
    for (size_t p = 0; p < nb; p++)
        if (pl.state[p] == PLACE_EMPTY) c.dropped[(size_t)ids[p]] = 1;
    commit(c, nullptr, &res.new_id);
    return res;
}

std::pair<int, uint32_t> MultiEngine::build_from_entries(const unsigned char *entries, const u64 *offsets)
{
    std::lock_guard<std::mutex> g(mu_);
    const uint32_t ipb = psu_.items_per_bundle, cap = psu_.table_params.max_items_per_bin - 1;
    const BulkPlan plan = devs_[0]->eng->entries_plan(offsets);    // every refusal of the plan comes before any GPU work
    if (plan.total > 0xFFFFFFFFull) throw std::invalid_argument("build_from_entries: more than 2^32 - 1 BinBundles");
    const std::vector<RegUnit> reg = registry_locked();
    for (const RegUnit &u : reg)
        if (plan.bundles[u.bundle_idx])
            throw std::invalid_argument("build_from_entries: bundle index " + std::to_string(u.bundle_idx) + " receives entries but holds a BinBundle already: "
                                        "entries are added to a database that exists with apply_entries");
    if (!entries && plan.total) throw std::invalid_argument("null argument");
    // the slots, in (b, k) order, the loads as each one registers
    std::vector<uint64_t> load = device_loads(reg, (int)devs_.size());
    std::vector<int> slot((size_t)plan.total);
    size_t at = 0;
    for (uint32_t b = 0; b < plan.bundles.size(); b++)
        for (uint32_t k = 0; k < plan.bundles[b]; k++, at++) {
            slot[at] = place_new_unit(b, psu_.bundle_idx_count, (int)devs_.size(), load.data());
            load[(size_t)slot[at]] += unit_cost(bulk_degree(offsets + (size_t)b * ipb, plan.kstart.data() + (size_t)b * ipb, ipb, k, cap));
        }
    std::vector<std::unique_ptr<Bundle>> built((size_t)plan.total);
    run_all([&](Dev &d) {
        std::vector<unsigned char> want((size_t)plan.total);
        bool any = false;
        for (size_t i = 0; i < want.size(); i++) any |= (want[i] = slot[i] == d.slot) != 0;
        if (!any) return;
        std::vector<std::unique_ptr<Bundle>> mine = d.eng->build_from_entries(entries, false, offsets, want.data());
        for (size_t i = 0; i < want.size(); i++)
            if (want[i]) built[i] = std::move(mine[i]);
    });
    Change c(reg.size());
    for (size_t i = 0; i < built.size(); i++) c.appended.push_back({ slot[i], std::move(built[i]) });
    commit(c, nullptr, nullptr);
    return { (int)reg.size(), (uint32_t)plan.total };
}

// one merged BinBundle per group (ids in cache order), made on merge_home; groups with different homes run side by side
std::vector<std::unique_ptr<Bundle>> MultiEngine::merge_groups(const std::vector<std::vector<int>> &groups)
{
    const std::vector<RegUnit> reg = registry_locked();
    std::vector<int> home(groups.size());
    std::vector<uint32_t> cache_idx(groups.size());
    for (size_t gi = 0; gi < groups.size(); gi++) {
        std::vector<RegUnit> members;
        for (int id : groups[gi]) members.push_back(reg.at((size_t)id));
        home[gi] = merge_home(members);
        cache_idx[gi] = members[merge_first(members)].cache_idx;
    }
    std::vector<std::unique_ptr<Bundle>> merged(groups.size());
    run_all([&](Dev &d) {
        for (size_t gi = 0; gi < groups.size(); gi++) {
            if (home[gi] != d.slot) continue;
            std::vector<std::unique_ptr<Bundle>> temporaries;
            std::vector<const Bundle *> bs;
            for (int id : groups[gi]) {
                const RegUnit &u = reg[(size_t)id];
                if (u.slot == d.slot) { bs.push_back(&bundle_locked(id)); continue; }
                temporaries.push_back(d.eng->clone_bundle(bundle_locked(id), devs_[(size_t)u.slot]->device));
                bs.push_back(temporaries.back().get());
            }
            merged[gi] = d.eng->merge_bundles(bs.data(), (uint32_t)bs.size(), cache_idx[gi]);
        }
    });
    return merged;
}

void MultiEngine::merge_bundles(const int *ids, uint32_t n_ids, int *new_id)
{
    std::lock_guard<std::mutex> g(mu_);
    if (n_ids < 2) throw std::invalid_argument("a merge takes at least two BinBundles");
    std::vector<int> members(ids, ids + n_ids);
    for (int id : members) check_id(id);
    const std::vector<RegUnit> reg = registry_locked();
    std::stable_sort(members.begin(), members.end(), [&](int a, int b) { return reg[(size_t)a].cache_idx < reg[(size_t)b].cache_idx; });
    for (size_t i = 1; i < members.size(); i++) {
        if (members[i] == members[i - 1]) throw std::invalid_argument("BinBundle " + std::to_string(members[i]) + " is named twice");
        if (reg[(size_t)members[i]].bundle_idx == reg[(size_t)members[i - 1]].bundle_idx && reg[(size_t)members[i]].cache_idx == reg[(size_t)members[i - 1]].cache_idx)
            throw std::invalid_argument("two BinBundles of the merge share a cache_idx");
    }
    std::vector<std::unique_ptr<Bundle>> merged = merge_groups({ members });
    Change c(reg.size());
    c.replaced[(size_t)members[0]] = std::move(merged[0]);
    for (size_t i = 1; i < members.size(); i++) c.dropped[(size_t)members[i]] = 1;
    commit(c, new_id, nullptr);
}

uint32_t MultiEngine::compact(uint32_t bundle_idx, int *new_id)
{
    std::lock_guard<std::mutex> g(mu_);
    const size_t n = hp_.n;
    devs_[0]->eng->lookup_counts("compact", nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr);             // the context's own refusals
    if (bundle_idx >= psu_.bundle_idx_count) throw std::invalid_argument("bundle_idx out of range");
    const std::vector<RegUnit> reg = registry_locked();
    const std::vector<int> ids = index_in_cache_order(reg, bundle_idx);
    const uint32_t nb = (uint32_t)ids.size();
    std::vector<std::vector<size_t>> mine(devs_.size());
    for (size_t p = 0; p < nb; p++) mine[(size_t)reg[(size_t)ids[p]].slot].push_back(p);
    std::vector<uint32_t> counts((size_t)nb * n);
    run_all([&](Dev &d) {
        const std::vector<size_t> &pos = mine[(size_t)d.slot];
        if (pos.empty()) return;
        std::vector<const Bundle *> bs;
        for (size_t p : pos) bs.push_back(&bundle_locked(ids[p]));
        std::vector<uint32_t> lc(pos.size() * n);
        d.eng->lookup_counts("compact", bs.data(), (uint32_t)bs.size(), nullptr, nullptr, 0, lc.data(), nullptr);
        for (size_t i = 0; i < pos.size(); i++)
            std::copy(lc.begin() + (std::ptrdiff_t)(i * n), lc.begin() + (std::ptrdiff_t)((i + 1) * n), counts.begin() + (std::ptrdiff_t)(pos[i] * n));
    });
    const CompactPlan plan = plan_compaction(counts.data(), nb, n, psu_.table_params.max_items_per_bin);
    std::vector<std::vector<int>> groups;
    for (size_t gi = 0; gi < plan.degree.size(); gi++) {
        std::vector<int> members;
        for (uint32_t p = 0; p < nb; p++)
            if (plan.group[p] == gi) members.push_back(ids[p]);
        if (members.size() >= 2) groups.push_back(std::move(members));
    }
    std::vector<std::unique_ptr<Bundle>> merged = merge_groups(groups);
    Change c(reg.size());
    for (size_t gi = 0; gi < groups.size(); gi++) {
        c.replaced[(size_t)groups[gi][0]] = std::move(merged[gi]);
        for (size_t i = 1; i < groups[gi].size(); i++) c.dropped[(size_t)groups[gi][i]] = 1;
    }
    commit(c, new_id, nullptr);
    return (uint32_t)groups.size();
}

} // namespace apsu_he
