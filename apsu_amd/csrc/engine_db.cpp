// See engine.h.  The calls on a resident database: a BinBundle updated, searched, listed, merged, split, moved to another context, built
// from the database's entries, exported in the reference's saved format, evaluated in plaintext and self-tested.  Each decodes what
// engine_bundles.cpp stored (decode_counted) and, where it makes a new BinBundle, ends in that file's encode_bundle.  One clock for all of
// them (op_times), one place for the context's refusals (lookup_check).
#include "engine_impl.h"

#include <chrono>

#include "db_rebase.h"
#include "seal_codec.h"
#include "wire.h"

namespace apsu_he {

void EventStamps::reserve(size_t count)
{
    while (ev.size() < count) {
        hipEvent_t e;
        HIP_CHECK(hipEventCreate(&e));
        ev.push_back(e);
    }
}
void EventStamps::record(size_t i, hipStream_t st) { HIP_CHECK(hipEventRecord(ev.at(i), st)); }
double EventStamps::ms(size_t from, size_t to) const
{
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, ev[from], ev[to]));
    return ms;
}
void EventStamps::release()
{
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    ev.clear();
}

void Engine::op_times(Op op, double *ms, int count)
{
    Enter g(this);
    for (int i = 0; i < count && i < OP_SPANS; i++) ms[i] = clock_[op].ms[i];
}

void Engine::lookup_check(const char *what, int need) const
{
    if (!has_psu_) throw std::logic_error("context was created without PSUParams");
    if (need >= NEED_BATCHING && !hp_.batching) throw std::logic_error("plain_modulus does not support batching");
    if (need >= NEED_DECODE && !unlift_exact_) throw std::logic_error("q_0 <= 2 * plain_modulus: stored plaintexts cannot be decoded");
    if (what && psu_.bins_per_bundle > hp_.n) throw std::logic_error(std::string(what) + ": more bins than batching slots");
}

u64 *Engine::decode_counted(const Bundle &b, uint32_t *dcounts, u64 *coeff, EventStamps *evs, size_t mid)
{
    const size_t n = hp_.n;
    u64 *poly = ws((size_t)(b.degree + 1) * n);                        // [d][slot] slot values of the batched polynomial
    const size_t mark = arena_off_;
    decode_bundle(b, poly, coeff);
    arena_off_ = mark;                                                 // the decode's workspace is free again (stream order)
    if (evs) evs->record(mid, st_);
    if (dcounts) launch_bin_counts(poly, n, b.degree + 1, dcounts, st_);
    return poly;
}

std::unique_ptr<Bundle> Engine::update_bundle(const Bundle &old, const u64 *ins_roots, const uint32_t *ins_counts, uint32_t ins_stride,
                                              const u64 *rem_roots, const uint32_t *rem_counts, uint32_t rem_stride, uint32_t bins)
{
    Enter g(this);
    TIER1_SLOTS();
    lookup_check(nullptr);
    const size_t n = hp_.n;
    if (bins > n) throw std::invalid_argument("more bins than batching slots");
    if ((ins_roots == nullptr) != (ins_counts == nullptr) || (rem_roots == nullptr) != (rem_counts == nullptr))
        throw std::invalid_argument("a root list and its counts are given together or not at all");
    const uint32_t max_items = psu_.table_params.max_items_per_bin;
    std::vector<uint32_t> touched;
    uint32_t max_ins = 0;
    for (uint32_t s = 0; s < bins; s++) {
        const uint32_t ni = ins_counts ? ins_counts[s] : 0, nr = rem_counts ? rem_counts[s] : 0;
        if (ni > ins_stride || nr > rem_stride) throw std::invalid_argument("bin count exceeds stride");
        if (ni > max_items) throw std::invalid_argument("bin size exceeds max_items_per_bin");
        if (ni) check_reduced(ins_roots + (size_t)s * ins_stride, ni, hp_.t, field_element);
        if (nr) check_reduced(rem_roots + (size_t)s * rem_stride, nr, hp_.t, field_element);
        max_ins = std::max(max_ins, ni);
        if (ni || nr) touched.push_back(s);
    }
    const uint32_t rows = old.degree + max_ins + 1;                    // no bin can outgrow this
    const size_t ins_words = ins_counts ? (size_t)bins * ins_stride : 0, rem_words = rem_counts ? (size_t)bins * rem_stride : 0;
    std::unique_ptr<Bundle> b;
    WITH_ARENA({
        u64 *poly = ws((size_t)rows * n);                              // [d][slot] slot values of the batched polynomial
        decode_bundle(old, poly);
        if (rows > old.degree + 1) HIP_CHECK(hipMemsetAsync(poly + (size_t)(old.degree + 1) * n, 0, (size_t)(rows - old.degree - 1) * n * sizeof(u64), st_));
        u64 *status = ws(3);                                           // failed removal, unused slot named (both atomicMin), degree (atomicMax)
        HIP_CHECK(hipMemsetAsync(status, 0xff, 2 * sizeof(u64), st_));
        HIP_CHECK(hipMemsetAsync(status + 2, 0, sizeof(u64), st_));
        std::vector<uint32_t> new_counts(touched.size());
        if (!touched.empty()) {
            u64 *dins = ws(ins_words + 1), *drem = ws(rem_words + 1);
            uint32_t *dic = ws_as<uint32_t>(bins, 1), *drc = ws_as<uint32_t>(bins, 1);
            uint32_t *dtouched = ws_as<uint32_t>(touched.size(), 1), *dnew = ws_as<uint32_t>(touched.size(), 1);
            if (ins_words) H2D(dins, ins_roots, ins_words);
            if (rem_words) H2D(drem, rem_roots, rem_words);
            if (ins_counts) HIP_CHECK(hipMemcpyAsync(dic, ins_counts, bins * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
            if (rem_counts) HIP_CHECK(hipMemcpyAsync(drc, rem_counts, bins * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
            HIP_CHECK(hipMemcpyAsync(dtouched, touched.data(), touched.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
            launch_bins_update(dtouched, (u32)touched.size(), dins, ins_counts ? dic : nullptr, ins_stride, drem, rem_counts ? drc : nullptr, rem_stride,
                               make_mod(hp_.t), poly, n, rows, dnew, status, st_);
            HIP_CHECK(hipMemcpyAsync(new_counts.data(), dnew, touched.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
        }
        launch_poly_degree(poly, n, rows, status + 2, st_);
        u64 st[3];
        HIP_CHECK(hipMemcpyAsync(st, status, sizeof(st), hipMemcpyDeviceToHost, st_));
        sync();                                                        // the new shape is decided on the host
        if (st[1] != ~(u64)0)
            throw std::invalid_argument("bin " + std::to_string(st[1]) + " is an unused slot (it holds the zero polynomial): nothing can be inserted or removed there");
        if (st[0] != ~(u64)0) {
            const uint32_t s = (uint32_t)(st[0] >> 32), r = (uint32_t)st[0];
            throw std::invalid_argument("bin " + std::to_string(s) + ": " + std::to_string(rem_roots[(size_t)s * rem_stride + r]) + " (removal " +
                                        std::to_string(r) + ") is not a root of the bin's polynomial");
        }
        uint32_t degree = (uint32_t)st[2];                             // untouched bins included (k_poly_degree)
        for (uint32_t c : new_counts) degree = std::max(degree, c);
        if (degree > max_items) throw std::invalid_argument("bin size exceeds max_items_per_bin");
        b = new_bundle(old.bundle_idx, old.cache_idx, degree);
        encode_bundle(*b, poly);
        sync();
    });
    pack_bundle(*b);
    return b;
}

// ---- N1, find and place: occupancy, membership and the database-level step on resident BinBundles
void Engine::lookup_impl(const Bundle *const *bundles, uint32_t n_bundles, const u64 *felts, const uint32_t *start, size_t count, uint32_t *counts,
                         unsigned char *flags)
{
    const size_t n = hp_.n;
    const uint32_t F = psu_.item_params.felts_per_item;
    if (count && count >= (size_t)LOOKUP_NONE / F) throw std::invalid_argument("too many entries for one call");
    for (size_t e = 0; e < count; e++) {
        if ((u64)start[e] + F > psu_.bins_per_bundle) throw std::invalid_argument("entry " + std::to_string(e) + ": start bin + felts_per_item exceeds bins_per_bundle");
        check_reduced(felts + e * F, F, hp_.t, [&](size_t, u64) { return "entry " + std::to_string(e) + ": field element"; });
    }
    const size_t parts = count * F;
    const LookupPlan plan = count ? lookup_plan(felts, start, count, F, n, LOOKUP_R) : LookupPlan();
    OpClock &clk = clock_[OP_LOOKUP];
    clk.evs.reserve((size_t)3 * n_bundles);                            // per BinBundle: before the decode, behind it, behind the kernels
    WITH_ARENA({
        LookupWork *dwork = nullptr;
        u64 *dpts = nullptr;
        uint32_t *didx = nullptr;
        if (count) {
            dwork = ws_as<LookupWork>(plan.work.size());
            dpts = ws(plan.pts.size());
            didx = ws_as<uint32_t>(plan.idx.size());
            HIP_CHECK(hipMemcpyAsync(dwork, plan.work.data(), plan.work.size() * sizeof(LookupWork), hipMemcpyHostToDevice, st_));
            HIP_CHECK(hipMemcpyAsync(dpts, plan.pts.data(), plan.pts.size() * sizeof(u64), hipMemcpyHostToDevice, st_));
            HIP_CHECK(hipMemcpyAsync(didx, plan.idx.data(), plan.idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
        }
        unsigned char *dflags = count ? ws_as<unsigned char>(parts) : nullptr;
        uint32_t *dcounts = counts ? ws_as<uint32_t>(n) : nullptr;
        const size_t mark = arena_off_;
        for (uint32_t i = 0; i < n_bundles; i++) {
            const Bundle &b = *bundles[i];
            arena_off_ = mark;                                         // one BinBundle after the other through the same workspace (stream order)
            clk.evs.record(3 * i, st_);
            const u64 *poly = decode_counted(b, dcounts, nullptr, &clk.evs, 3 * i + 1);
            if (counts) HIP_CHECK(hipMemcpyAsync(counts + (size_t)i * n, dcounts, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
            if (count) {
                launch_bins_lookup(dwork, (u32)plan.work.size(), dpts, didx, make_mod(hp_.t), poly, n, b.degree, dflags, st_);
                HIP_CHECK(hipMemcpyAsync(flags + (size_t)i * parts, dflags, parts, hipMemcpyDeviceToHost, st_));
            }
            clk.evs.record(3 * i + 2, st_);
        }
        sync();
    });
    clk.ms[0] = clk.ms[1] = 0;
    for (uint32_t i = 0; i < n_bundles; i++)
        for (int k = 0; k < 2; k++) clk.ms[k] += clk.evs.ms(3 * i + k, 3 * i + k + 1);
}

void Engine::bin_counts(const Bundle &b, uint32_t *counts)
{
    Enter g(this);
    TIER1_SLOTS();
    lookup_check("bin_counts");
    const Bundle *one = &b;
    lookup_impl(&one, 1, nullptr, nullptr, 0, counts, nullptr);
}

// present[b][e] = AND over the entry's parts; room[b][e] = max_j(count[s + j] + 1), multi_insert_dry_run's return value, or LOOKUP_NONE
static void lookup_reduce(const unsigned char *flags, const uint32_t *counts, uint32_t n_bundles, size_t n, const uint32_t *start, size_t count, uint32_t F,
                          unsigned char *present, uint32_t *room)
{
    for (uint32_t b = 0; b < n_bundles; b++)
        for (size_t e = 0; e < count; e++) {
            unsigned char all = 1;
            uint32_t most = 0;
            for (uint32_t j = 0; j < F; j++) {
                all &= flags[((size_t)b * count + e) * F + j];
                const uint32_t c = counts[(size_t)b * n + start[e] + j];
                most = most == LOOKUP_NONE || c == LOOKUP_NONE ? LOOKUP_NONE : std::max(most, c + 1);
            }
            if (present) present[(size_t)b * count + e] = all;
            if (room) room[(size_t)b * count + e] = most;
        }
}

void Engine::lookup_bundles(const Bundle *const *bundles, uint32_t n_bundles, const u64 *felts, const uint32_t *start, size_t count,
                            unsigned char *present, uint32_t *room)
{
    Enter g(this);
    TIER1_SLOTS();
    lookup_check("lookup");
    if (!n_bundles || !count) return;
    const size_t n = hp_.n;
    const uint32_t F = psu_.item_params.felts_per_item;
    std::vector<unsigned char> flags((size_t)n_bundles * count * F);
    std::vector<uint32_t> counts((size_t)n_bundles * n);
    lookup_impl(bundles, n_bundles, felts, start, count, counts.data(), flags.data());
    lookup_reduce(flags.data(), counts.data(), n_bundles, n, start, count, F, present, room);
}

void Engine::lookup_counts(const char *what, const Bundle *const *bundles, uint32_t n_bundles, const u64 *felts, const uint32_t *start, size_t count,
                           uint32_t *counts, unsigned char *present)
{
    Enter g(this);
    TIER1_SLOTS();
    lookup_check(what);
    if (!n_bundles) return;
    const size_t n = hp_.n;
    const uint32_t F = psu_.item_params.felts_per_item;
    std::vector<unsigned char> flags((size_t)n_bundles * count * F);
    lookup_impl(bundles, n_bundles, felts, start, count, counts, count ? flags.data() : nullptr);
    if (count) lookup_reduce(flags.data(), counts, n_bundles, n, start, count, F, present, nullptr);
}

// ---- N1, reading the bins back (bin_roots.h): decode, k_bin_counts, k_bin_roots (or the per-coset composition), k_roots_mult, one sync,
// then the host's sort per bin and the sum check
void Engine::roots_tables()
{
    if (roots_g_) return;
    const size_t n = hp_.n;
    const u64 g = field_generator(hp_.t);
    const std::vector<u32> step = roots_step_table(g, hp_.t, n);
    d_roots_step_.alloc(n * sizeof(u32));
    HIP_CHECK(hipMemcpy(d_roots_step_.p(), step.data(), n * sizeof(u32), hipMemcpyHostToDevice));
    // the evaluation point of output position k is the transform of X at k: the output order is the launch's own
    d_roots_pts_.alloc(n * sizeof(u64));
    std::vector<u64> x(n, 0);
    x[1] = 1;
    HIP_CHECK(hipMemcpy(d_roots_pts_.p(), x.data(), n * sizeof(u64), hipMemcpyHostToDevice));
    d_ntt(d_roots_pts_.u(), 1, map_ct() + hp_.plain_id(), 1, false, false);
    sync();
    roots_g_ = g;
}

bool Engine::bins_prepare(const Bundle &b, int form)
{
    lookup_check("bins");
    const size_t n = hp_.n;
    roots_coset_count(hp_.t, n);                                       // (refuses a plain modulus with too many cosets)
    if (b.degree >= n) throw std::logic_error("bins: a bin's polynomial of degree " + std::to_string(b.degree) + " does not fit one transform of " + std::to_string(n) + " points");
    const bool has_kernel = bin_roots_has_kernel(hp_.logn);
    if (form == BINS_FORM_KERNEL && !has_kernel) throw std::logic_error("bins: no persistent kernel for this ring size");
    roots_tables();
    return form == BINS_FORM_COMPOSED ? false : has_kernel;
}

Engine::BinsCounted Engine::bins_counted(const Bundle &b, bool want_coeff, uint32_t *counts, EventStamps &evs)
{
    const size_t n = hp_.n;
    evs.record(0, st_);
    BinsCounted c{ nullptr, nullptr, ws_as<uint32_t>(n), counts };
    if (want_coeff) c.coeff = ws((size_t)(b.degree + 1) * n);
    c.poly = decode_counted(b, c.dcounts, c.coeff);
    HIP_CHECK(hipMemcpyAsync(counts, c.dcounts, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
    evs.record(1, st_);
    sync();                                                            // which bins are occupied, and the lists' size, are decided on the host
    return c;
}

void Engine::bins_search(const BinsCounted &c, bool kernel, const uint32_t *stride, EventStamps &evs, size_t s, BinsFound &f)
{
    const BinsDevice d = bins_search_device(c, kernel, stride, evs, s, f);
    const u32 n_occ = (u32)f.occ.size();
    if (n_occ) {
        f.hits.resize((size_t)n_occ * f.hstride); f.found.resize(n_occ); f.mult.resize((size_t)n_occ * f.hstride);
        HIP_CHECK(hipMemcpyAsync(f.found.data(), d.found, n_occ * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
        HIP_CHECK(hipMemcpyAsync(f.mult.data(), d.mult, f.mult.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
        HIP_CHECK(hipMemcpyAsync(f.hits.data(), d.hits, f.hits.size() * sizeof(u64), hipMemcpyDeviceToHost, st_));
    }
    evs.record(s + 1, st_);
}

Engine::BinsDevice Engine::bins_search_device(const BinsCounted &c, bool kernel, const uint32_t *stride, EventStamps &evs, size_t s, BinsFound &f)
{
    BinsDevice d{ nullptr, nullptr, nullptr, nullptr };
    const size_t n = hp_.n;
    const u32 cosets = roots_coset_count(hp_.t, n);
    const Mod t = make_mod(hp_.t);
    const u32 *step = reinterpret_cast<const u32 *>(d_roots_step_.p());
    const u64 *pts = d_roots_pts_.u();
    for (size_t i = 0; i < n; i++)
        if (c.counts[i] != LOOKUP_NONE && c.counts[i] >= 1) { f.occ.push_back((uint32_t)i); f.hstride = std::max(f.hstride, c.counts[i]); }
    const uint32_t hstride = f.hstride;
    if (stride && *stride < hstride) throw std::invalid_argument("bins: stride " + std::to_string(*stride) + " is below the largest bin count " + std::to_string(hstride));
    const u32 n_occ = (u32)f.occ.size();
    if (n_occ) {
        uint32_t *docc = ws_as<uint32_t>(n_occ), *dfound = ws_as<uint32_t>(n_occ), *dmult = ws_as<uint32_t>((size_t)n_occ * hstride);
        u64 *dhits = ws((size_t)n_occ * hstride);
        HIP_CHECK(hipMemcpyAsync(docc, f.occ.data(), n_occ * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
        HIP_CHECK(hipMemsetAsync(dfound, 0, n_occ * sizeof(uint32_t), st_));
        if (kernel) {
            const u32 slots = bin_roots_wg_slots(hp_.logn);
            const RootsGrid grid = roots_grid(n_occ, cosets, slots);
            const u32 wgs = (u32)std::min<u64>((u64)n_occ * grid.blocks, slots);
            u64 *rows = ws((size_t)wgs * n);
            u32 *vrows = ws_as<u32>((size_t)wgs * n);
            launch_bin_roots(hp_.logn, c.poly, docc, c.dcounts, n_occ, grid, cosets, wgs, tabs(), map_ct() + hp_.plain_id(), step, pts, roots_g_, rows, vrows,
                             dhits, dfound, hstride, st_);
        } else {
            // limb rows of at most 64 MiB at a time, all cosets for one group of bins, then the next group
            const u32 group = (u32)std::max<size_t>(1, std::min<size_t>(n_occ, ((size_t)64 << 20) / (n * sizeof(u64))));
            u64 *rows = ws((size_t)group * n);
            const u64 r1 = t.r1;
            for (u32 r0 = 0; r0 < n_occ; r0 += group) {
                const u32 nr = std::min(group, n_occ - r0);
                u64 cs = 1;
                for (u32 j = 0; j < cosets; j++) {
                    launch_roots_gather(c.poly, n, docc + r0, c.dcounts, nr, cs, t, rows, st_);
                    d_ntt(rows, nr, map_ct() + hp_.plain_id(), 1, false, false);
                    launch_roots_scan(rows, n, nr, pts, cs, t, j == 0, c.poly, docc + r0, c.dcounts, dhits + (size_t)r0 * hstride, dfound + r0, hstride, st_);
                    cs = roots_mul(cs, roots_g_, hp_.t, r1);
                }
            }
        }
        evs.record(s, st_);
        launch_roots_mult(c.poly, n, docc, c.dcounts, n_occ, t, dhits, dfound, dmult, hstride, st_);
        d = BinsDevice{ docc, dfound, dmult, dhits };
    } else evs.record(s, st_);
    return d;
}

// multiplicities (1 wherever a bin has as many distinct roots as items), the sum check, the sort; nothing is written to `roots` before
// every bin has passed
void Engine::bins_finish(const BinsCounted &c, BinsFound &f, u64 *roots, uint32_t stride)
{
    std::vector<std::vector<u64>> bins(f.occ.size());
    for (size_t r = 0; r < f.occ.size(); r++) {
        const u32 cnt = c.counts[f.occ[r]], nf = f.found[r];
        u32 *m = f.mult.data() + r * f.hstride;
        if (nf >= cnt) std::fill(m, m + std::min(nf, cnt), 1u);
        roots_expand(f.occ[r], cnt, f.hits.data() + r * f.hstride, m, nf, bins[r]);
    }
    if (!roots) return;
    for (size_t r = 0; r < f.occ.size(); r++) std::copy(bins[r].begin(), bins[r].end(), roots + (size_t)f.occ[r] * stride);
}

void Engine::bundle_bins(const Bundle &b, u64 *roots, uint32_t *counts, uint32_t stride, int form)
{
    Enter g(this);
    TIER1_SLOTS();
    const bool kernel = bins_prepare(b, form);
    OpClock &clk = clock_[OP_BINS];
    clk.evs.reserve(4);
    BinsCounted c{};
    BinsFound f;
    WITH_ARENA({
        f = BinsFound();                                               // (the body runs again after an arena overflow)
        c = bins_counted(b, false, counts, clk.evs);
        bins_search(c, kernel, roots ? &stride : nullptr, clk.evs, 2, f);
        sync();
    });
    for (int i = 0; i < 3; i++) clk.ms[i] = clk.evs.ms(i, i + 1);
    bins_finish(c, f, roots, stride);
}

// ---- N1, splitting (bin_split.h): bundle_bins' decode, counts and root search, k_roots_split, one sync and the failure word, then the
// tail of the build per part on the device-resident lists
std::vector<std::unique_ptr<Bundle>> Engine::split_bundle(const Bundle &b, uint32_t k, const uint32_t *cache_idx)
{
    Enter g(this);
    TIER1_SLOTS();
    if (k < 1) throw std::invalid_argument("split: a BinBundle is split into 1 part or more, not " + std::to_string(k));
    const bool kernel = bins_prepare(b, BINS_FORM_AUTO);
    const size_t n = hp_.n;
    OpClock &clk = clock_[OP_SPLIT];
    // stamps: 0, 1 around decode and counts (bins_counted); 2 in front of the root search, 3 behind it, 4 behind the multiplicities, 5
    // behind k_roots_split, 6 behind the builds
    clk.evs.reserve(7);
    std::vector<uint32_t> counts(n);
    std::vector<std::unique_ptr<Bundle>> parts;
    WITH_ARENA({
        parts.clear();                                                 // (the body runs again after an arena overflow)
        BinsFound f;
        const BinsCounted c = bins_counted(b, false, counts.data(), clk.evs);
        uint32_t bins = 0, most = 0;
        for (size_t s = 0; s < n; s++) {
            if (counts[s] == LOOKUP_NONE) continue;
            if (s != bins)
                throw std::invalid_argument("split: slot " + std::to_string(s) + " is a bin but slot " + std::to_string(bins) + " is not: the parts are built from a prefix of the slots");
            bins++;
            most = std::max(most, counts[s]);
        }
        if (most >= 1 && k > most)
            throw std::invalid_argument("split: " + std::to_string(k) + " parts, but the largest bin holds " + std::to_string(most) + " items: a part would be empty in every bin");
        const SplitShape shape = split_shape(counts.data(), n, k, LOOKUP_NONE);
        clk.evs.record(2, st_);
        const BinsDevice d = bins_search_device(c, kernel, nullptr, clk.evs, 3, f);      // (divides the columns of poly)
        clk.evs.record(4, st_);
        const u32 n_occ = (u32)f.occ.size();
        std::vector<u64> off(k);
        size_t words = 0;
        for (uint32_t p = 0; p < k; p++) { off[p] = words; words += (size_t)bins * shape.degree[p]; }
        u64 *dout = ws(words + 1), *doff = ws(k), *dfail = ws(1);
        u32 *dstride = ws_as<u32>(k, 1), *dpart_counts = ws_as<u32>((size_t)k * n, 1);
        HIP_CHECK(hipMemcpyAsync(doff, off.data(), k * sizeof(u64), hipMemcpyHostToDevice, st_));
        HIP_CHECK(hipMemcpyAsync(dstride, shape.degree.data(), k * sizeof(u32), hipMemcpyHostToDevice, st_));     // a part's stride is its degree
        HIP_CHECK(hipMemsetAsync(dfail, 0xff, sizeof(u64), st_));
        launch_roots_split(d.hits, d.found, d.mult, f.hstride, d.occ, c.dcounts, n_occ, k, dout, doff, dstride, dpart_counts, (u32)n, dfail, st_);
        clk.evs.record(5, st_);
        u64 failure = SPLIT_NO_FAILURE;
        HIP_CHECK(hipMemcpyAsync(&failure, dfail, sizeof(u64), hipMemcpyDeviceToHost, st_));
        sync();                                                        // nothing is built before every bin has passed
        if (failure != SPLIT_NO_FAILURE) {
            const uint32_t s = (uint32_t)(failure >> 32);
            throw std::invalid_argument("bin " + std::to_string(s) + ": its polynomial of degree " + std::to_string(counts[s]) + " does not split into linear factors (" +
                                        std::to_string((uint32_t)failure) + " roots found, counted with multiplicity)");
        }
        const size_t mark = arena_off_;
        for (uint32_t p = 0; p < k; p++) {
            arena_off_ = mark;                                         // one part after the other through the same workspace (stream order)
            parts.push_back(new_bundle(b.bundle_idx, cache_idx ? cache_idx[p] : b.cache_idx + p, shape.degree[p]));
            build_from_roots(*parts.back(), dout + off[p], dpart_counts + (size_t)p * n, bins, shape.degree[p]);
        }
        clk.evs.record(6, st_);
        sync();
    });
    for (auto &p : parts) pack_bundle(*p);
    const int span[4][2] = { { 0, 1 }, { 2, 4 }, { 4, 5 }, { 5, 6 } };
    for (int i = 0; i < 4; i++) clk.ms[i] = clk.evs.ms(span[i][0], span[i][1]);
    return parts;
}

// ---- N1, moving (db_rebase.h)
void Engine::export_coeff(const Bundle &b, DevBuf &raw)
{
    Enter g(this);
    TIER1_SLOTS();
    lookup_check(nullptr, NEED_DECODE);
    raw.alloc((size_t)(b.degree + 1) * hp_.n * sizeof(u64));
    WITH_ARENA({
        decode_coeff(b, raw.u());
        sync();
    });
}

std::unique_ptr<Bundle> Engine::adopt_bundle(Engine &src, const Bundle &b, uint32_t cache_idx)
{
    // the parameters never change: read without either lock
    if (!has_psu_ || !src.has_psu_) throw std::logic_error("context was created without PSUParams");
    if (src.device_ != device_)
        throw std::invalid_argument("adopt: the source context is on device " + std::to_string(src.device_) + ", this one on device " + std::to_string(device_) +
                                    ": BinBundles move between contexts of one device");
    const std::string why = rebase_compatible(src.psu_, psu_);
    if (!why.empty()) throw std::invalid_argument("adopt: " + why);
    const uint32_t max_items = psu_.table_params.max_items_per_bin;
    if (b.degree > max_items)
        throw std::invalid_argument("adopt: the BinBundle has degree " + std::to_string(b.degree) + ", above the destination's max_items_per_bin = " + std::to_string(max_items) +
                                    ": split it into " + std::to_string(split_parts(b.degree, max_items)) + " parts in the source first");
    DevBuf raw;                                                        // [degree+1][n] coefficient-form plaintexts mod t, this call's own
    src.export_coeff(b, raw);                                          // the source's lock, released on return
    Enter g(this);
    TIER1_SLOTS();
    lookup_check(nullptr, NEED_BATCHING);
    std::unique_ptr<Bundle> out;
    WITH_ARENA({
        out = new_bundle(b.bundle_idx, cache_idx, b.degree);
        finish_bundle(*out, raw.u());
        sync();
    });
    pack_bundle(*out);
    return out;
}

Engine::RebaseResult Engine::rebase_from(Engine &src, const Bundle *const *bundles, uint32_t n_bundles)
{
    if (!has_psu_ || !src.has_psu_) throw std::logic_error("context was created without PSUParams");
    const std::string why = rebase_compatible(src.psu_, psu_);
    if (!why.empty()) throw std::invalid_argument("rebase: " + why);
    const size_t n = src.hp_.n;
    std::vector<uint32_t> counts(n), most(n_bundles, 0), index(n_bundles);
    for (uint32_t i = 0; i < n_bundles; i++) {
        src.bin_counts(*bundles[i], counts.data());
        for (size_t s = 0; s < n; s++)
            if (counts[s] != LOOKUP_NONE) most[i] = std::max(most[i], counts[s]);
        index[i] = bundles[i]->bundle_idx;
    }
    const RebasePlan plan = rebase_plan(most.data(), index.data(), n_bundles, psu_.table_params.max_items_per_bin);
    RebaseResult res;                                                  // (a refusal below releases every BinBundle made so far with it)
    for (uint32_t i = 0; i < n_bundles; i++) {
        const uint32_t first = plan.first[i];
        if (plan.parts[i] == 1) res.bundles.push_back(adopt_bundle(src, *bundles[i], plan.cache_idx[first]));
        else {
            const std::vector<std::unique_ptr<Bundle>> parts = src.split_bundle(*bundles[i], plan.parts[i], nullptr);
            for (uint32_t p = 0; p < plan.parts[i]; p++) res.bundles.push_back(adopt_bundle(src, *parts[p], plan.cache_idx[first + p]));
        }
    }
    res.origin = plan.origin;
    return res;
}

// apply_entries and compact take the BinBundles of one bundle index, in cache order
static void check_one_index_in_cache_order(uint32_t bundle_idx, const Bundle *const *bundles, uint32_t n_bundles)
{
    for (uint32_t b = 0; b < n_bundles; b++) {
        if (bundles[b]->bundle_idx != bundle_idx) throw std::invalid_argument("the BinBundles of one call belong to one bundle index");
        if (b && bundles[b]->cache_idx <= bundles[b - 1]->cache_idx) throw std::invalid_argument("BinBundles are not in cache order");
    }
}

PlaceResult place_from_lookup(uint32_t n_bundles, size_t n, uint32_t bins, uint32_t F, uint32_t max_items, u64 t, const uint32_t *counts,
                              const unsigned char *present, const u64 *ins_felts, const uint32_t *ins_start, size_t n_ins, const u64 *rem_felts,
                              const uint32_t *rem_start, size_t n_rem)
{
    const size_t count = n_rem + n_ins;
    std::vector<uint32_t> bin_counts((size_t)n_bundles * bins);
    std::vector<unsigned char> ins_present((size_t)n_bundles * n_ins), rem_present((size_t)n_bundles * n_rem);
    for (uint32_t b = 0; b < n_bundles; b++) {
        std::copy(counts + (size_t)b * n, counts + (size_t)b * n + bins, bin_counts.begin() + (size_t)b * bins);
        std::copy(present + (size_t)b * count, present + (size_t)b * count + n_rem, rem_present.begin() + (size_t)b * n_rem);
        std::copy(present + (size_t)b * count + n_rem, present + (size_t)(b + 1) * count, ins_present.begin() + (size_t)b * n_ins);
    }
    PlaceInput in;
    in.n_bundles = n_bundles; in.bins = bins; in.F = F; in.max_items = max_items; in.t = t;
    in.counts = bin_counts.data(); in.ins_present = ins_present.data(); in.rem_present = rem_present.data();
    in.ins_felts = ins_felts; in.ins_start = ins_start; in.n_ins = n_ins;
    in.rem_felts = rem_felts; in.rem_start = rem_start; in.n_rem = n_rem;
    return place_entries(in);
}

Engine::ApplyResult Engine::apply_entries(uint32_t bundle_idx, const Bundle *const *bundles, uint32_t n_bundles, const u64 *ins_felts,
                                          const uint32_t *ins_start, size_t n_ins, const u64 *rem_felts, const uint32_t *rem_start, size_t n_rem)
{
    ApplyResult res;
    const size_t n = hp_.n;
    uint32_t F = 0, bins = 0;
    std::vector<uint32_t> counts;
    {
        Enter g(this);
        TIER1_SLOTS();
        lookup_check("apply_entries");
        F = psu_.item_params.felts_per_item;
        bins = psu_.bins_per_bundle;
        if (bundle_idx >= psu_.bundle_idx_count) throw std::invalid_argument("bundle_idx out of range");
        check_one_index_in_cache_order(bundle_idx, bundles, n_bundles);
        // the refusals come before any GPU work
        place_validate(ins_felts, ins_start, n_ins, rem_felts, rem_start, n_rem, F, bins, hp_.t);
        // one lookup for both lists: removals first, insertions behind them
        std::vector<u64> felts((n_rem + n_ins) * F);
        std::vector<uint32_t> start(n_rem + n_ins);
        std::copy(rem_felts, rem_felts + n_rem * F, felts.begin());
        std::copy(ins_felts, ins_felts + n_ins * F, felts.begin() + n_rem * F);
        std::copy(rem_start, rem_start + n_rem, start.begin());
        std::copy(ins_start, ins_start + n_ins, start.begin() + n_rem);
        const size_t count = n_rem + n_ins;
        std::vector<unsigned char> flags((size_t)n_bundles * count * F), present((size_t)n_bundles * count);
        counts.assign((size_t)n_bundles * n, 0);
        if (n_bundles) {
            lookup_impl(bundles, n_bundles, felts.data(), start.data(), count, counts.data(), count ? flags.data() : nullptr);
            lookup_reduce(flags.data(), counts.data(), n_bundles, n, start.data(), count, F, present.data(), nullptr);
        }
        res.place = place_from_lookup(n_bundles, n, bins, F, psu_.table_params.max_items_per_bin, hp_.t, counts.data(), present.data(), ins_felts,
                                      ins_start, n_ins, rem_felts, rem_start, n_rem);
    }
    // the context's lock is taken per step from here on, as by a caller who made these calls one by one; the given BinBundles are only read
    const PlaceResult &pl = res.place;
    res.replaced.resize(n_bundles);
    for (uint32_t b = 0; b < n_bundles; b++) {
        if (pl.state[b] != PLACE_REPLACED) continue;
        const PlaceLists &li = pl.ins[b], &lr = pl.rem[b];
        res.replaced[b] = update_bundle(*bundles[b], li.any() ? li.roots.data() : nullptr, li.any() ? li.counts.data() : nullptr, li.stride,
                                        lr.any() ? lr.roots.data() : nullptr, lr.any() ? lr.counts.data() : nullptr, lr.stride, bins);
    }
    const uint32_t next_cache = n_bundles ? bundles[n_bundles - 1]->cache_idx + 1 : 0;
    for (uint32_t k = 0; k < pl.n_new; k++) {
        const PlaceLists &li = pl.ins[n_bundles + k];
        res.appended.push_back(build_bundle(bundle_idx, next_cache + k, li.roots.data(), li.counts.data(), bins, li.stride));
    }
    return res;
}

// ---- N1, a whole database from its entries (bulk_place.h): per bundle index one copy of its entries, per BinBundle k_entries_scatter
// and the tail of the build on the device-resident lists
BulkPlan Engine::entries_plan(const u64 *offsets) const
{
    // the parameters never change: read without the lock
    if (!has_psu_) throw std::logic_error("context was created without PSUParams");
    return bulk_plan(offsets, psu_.table_params.table_size, psu_.items_per_bundle, psu_.table_params.max_items_per_bin);
}

std::vector<std::unique_ptr<Bundle>> Engine::build_from_entries(const unsigned char *entries, bool on_device, const u64 *offsets, const unsigned char *want)
{
    Enter g(this);
    TIER1_SLOTS();
    lookup_check("build_from_entries", NEED_BATCHING);
    const size_t n = hp_.n;
    const u32 ipb = psu_.items_per_bundle, F = psu_.item_params.felts_per_item, bins = psu_.bins_per_bundle, cap = psu_.table_params.max_items_per_bin - 1;
    const BulkPlan plan = bulk_plan(offsets, psu_.table_params.table_size, ipb, psu_.table_params.max_items_per_bin);   // every refusal comes before any GPU work
    if (plan.total > 0xFFFFFFFFull) throw std::invalid_argument("build_from_entries: more than 2^32 - 1 BinBundles");
    OpClock &clk = clock_[OP_BUILD];
    // stamps: per bundle index two around the copies, per BinBundle three: in front of the scatter, behind it, behind the build
    clk.evs.reserve(2 * plan.bundles.size() + 3 * (size_t)plan.total);
    for (double &m : clk.ms) m = 0;
    std::vector<std::unique_ptr<Bundle>> out((size_t)plan.total);
    size_t at = 0, stamp = 0;
    for (u32 b = 0; b < plan.bundles.size(); at += plan.bundles[b], b++) {
        const u32 K = plan.bundles[b];
        bool any = false;
        for (u32 k = 0; k < K; k++) any |= !want || want[at + k];
        if (!any) continue;
        const u64 *off = offsets + (size_t)b * ipb;
        const u32 *kstart = plan.kstart.data() + (size_t)b * ipb;
        const size_t count = off[ipb] - off[0];
        const size_t first_stamp = stamp;
        WITH_ARENA({
            stamp = first_stamp;                                       // (the body runs again after an arena overflow)
            clk.evs.record(stamp++, st_);
            unsigned char *ditems = ws_as<unsigned char>(count * 16 + 16);
            HIP_CHECK(hipMemcpyAsync(ditems, entries + off[0] * 16, count * 16, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st_));
            u64 *doff = ws((size_t)ipb + 1);
            u32 *dkstart = ws_as<u32>(ipb, 1);
            HIP_CHECK(hipMemcpyAsync(doff, off, ((size_t)ipb + 1) * sizeof(u64), hipMemcpyHostToDevice, st_));
            HIP_CHECK(hipMemcpyAsync(dkstart, kstart, (size_t)ipb * sizeof(u32), hipMemcpyHostToDevice, st_));
            clk.evs.record(stamp++, st_);
            const size_t mark = arena_off_;
            for (u32 k = 0; k < K; k++) {
                if (want && !want[at + k]) continue;
                arena_off_ = mark;                                     // one BinBundle after the other through the same workspace (stream order)
                const u32 degree = bulk_degree(off, kstart, ipb, k, cap), stride = std::max<u32>(1, degree);
                out[at + k] = new_bundle(b, k, degree);
                u64 *droots = ws((size_t)bins * stride + 1);
                u32 *dcounts = ws_as<u32>(n, 1);
                clk.evs.record(stamp++, st_);
                launch_entries_scatter(ditems, doff, dkstart, ipb, F, psu_.item_bit_count_per_felt, psu_.item_bit_count, cap, k, stride, droots, dcounts, (u32)n, scatter_blocks_, st_);
                clk.evs.record(stamp++, st_);
                build_from_roots(*out[at + k], droots, dcounts, bins, stride);
                clk.evs.record(stamp++, st_);
            }
            sync();
        });
        clk.ms[0] += clk.evs.ms(first_stamp, first_stamp + 1);
        for (size_t s = first_stamp + 2; s < stamp; s += 3) { clk.ms[1] += clk.evs.ms(s, s + 1); clk.ms[2] += clk.evs.ms(s + 1, s + 2); }
        for (u32 k = 0; k < K; k++)
            if (out[at + k]) pack_bundle(*out[at + k]);
    }
    return out;
}

// ---- N1, compaction: several BinBundles of one bundle index into one (bin_merge.h, db_compact.h)
std::unique_ptr<Bundle> Engine::merge_bundles(const Bundle *const *bundles, uint32_t n_bundles, uint32_t cache_idx)
{
    Enter g(this);
    TIER1_SLOTS();
    lookup_check("merge");
    if (n_bundles < 2) throw std::invalid_argument("a merge takes at least two BinBundles");
    for (uint32_t i = 1; i < n_bundles; i++)
        if (bundles[i]->bundle_idx != bundles[0]->bundle_idx)
            throw std::invalid_argument("BinBundle " + std::to_string(i) + " belongs to bundle index " + std::to_string(bundles[i]->bundle_idx) +
                                        ", the first to " + std::to_string(bundles[0]->bundle_idx));
    const size_t n = hp_.n, tiles = (n + MERGE_LANES - 1) / MERGE_LANES;
    const uint32_t steps = n_bundles - 1;
    std::vector<uint32_t> degrees(n_bundles);
    for (uint32_t i = 0; i < n_bundles; i++) degrees[i] = bundles[i]->degree;
    std::unique_ptr<Bundle> b;
    OpClock &clk = clock_[OP_MERGE];
    clk.evs.reserve(5);
    WITH_ARENA({
        clk.evs.record(0, st_);
        uint32_t *dcounts = ws_as<uint32_t>((size_t)n_bundles * n);
        std::vector<const u64 *> poly(n_bundles);                      // [d][slot] slot values, one array per BinBundle
        for (uint32_t i = 0; i < n_bundles; i++) poly[i] = decode_counted(*bundles[i], dcounts + (size_t)i * n);
        std::vector<uint32_t> counts((size_t)n_bundles * n);
        HIP_CHECK(hipMemcpyAsync(counts.data(), dcounts, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
        clk.evs.record(1, st_);
        sync();                                                        // what may be merged, and every step's shape, is decided on the host
        // step k multiplies the product of BinBundles 0 .. k by BinBundle k + 1; every refusal comes before the first product
        const MergeSteps ms = merge_steps(counts.data(), degrees.data(), n_bundles, n, psu_.table_params.max_items_per_bin);
        int *dtops = ws_as<int>(ms.tops.size());
        HIP_CHECK(hipMemcpyAsync(dtops, ms.tops.data(), ms.tops.size() * sizeof(int), hipMemcpyHostToDevice, st_));
        const uint32_t most_rows = *std::max_element(ms.rows.begin(), ms.rows.end());     // (an early step can be the tallest: merge_steps)
        u64 *buf[2] = { ws((size_t)most_rows * n), steps > 1 ? ws((size_t)most_rows * n) : nullptr };
        clk.evs.record(2, st_);
        const u64 *cur = poly[0];
        for (uint32_t k = 0; k < steps; k++) {
            u64 *out = buf[(steps - 1 - k) & 1];                       // the last step writes buf[0]
            launch_bins_merge(cur, dtops + (size_t)2 * k * tiles, poly[k + 1], dtops + (size_t)(2 * k + 1) * tiles, make_mod(hp_.t), out, n, ms.rows[k], st_);
            cur = out;
        }
        clk.evs.record(3, st_);
        b = new_bundle(bundles[0]->bundle_idx, cache_idx, ms.degree);
        encode_bundle(*b, cur);                                        // rows above `degree` are 0: rows[] is a bound over tiles, degree over slots
        clk.evs.record(4, st_);
        sync();
    });
    pack_bundle(*b);
    const int span[3][2] = { { 0, 1 }, { 2, 3 }, { 3, 4 } };
    for (int i = 0; i < 3; i++) clk.ms[i] = clk.evs.ms(span[i][0], span[i][1]);
    return b;
}

Engine::CompactResult Engine::compact(uint32_t bundle_idx, const Bundle *const *bundles, uint32_t n_bundles)
{
    CompactResult res;
    const size_t n = hp_.n;
    {
        Enter g(this);
        TIER1_SLOTS();
        lookup_check("compact");
        if (bundle_idx >= psu_.bundle_idx_count) throw std::invalid_argument("bundle_idx out of range");
        check_one_index_in_cache_order(bundle_idx, bundles, n_bundles);
        std::vector<uint32_t> counts((size_t)n_bundles * n);
        if (n_bundles) lookup_impl(bundles, n_bundles, nullptr, nullptr, 0, counts.data(), nullptr);
        res.plan = plan_compaction(counts.data(), n_bundles, n, psu_.table_params.max_items_per_bin);
    }
    // the context's lock is taken per merge from here on, as by a caller who made these calls one by one; the given BinBundles are only read
    res.merged.resize(res.plan.degree.size());
    for (size_t g = 0; g < res.merged.size(); g++) {
        std::vector<const Bundle *> members;
        for (uint32_t b = 0; b < n_bundles; b++)
            if (res.plan.group[b] == g) members.push_back(bundles[b]);
        if (members.size() >= 2) res.merged[g] = merge_bundles(members.data(), (uint32_t)members.size(), members[0]->cache_idx);
    }
    return res;
}

// ---- N2 towards the reference: a resident BinBundle as BinBundle::save writes it (wire.h: build_bin_bundle; bin_rows.h)
void Engine::keep_coeff_rows(const Bundle &b, const u64 *coeff, DevBuf &keep)
{
    const size_t n = hp_.n;
    const size_t H = b.use_ps ? b.H : 0;
    keep.alloc((H + 1) * n * sizeof(u64));
    D2D(keep.u(), coeff, n);
    for (const BundleRun &r : layout_of(b.degree).runs)
        if (r.kind == COEFF_LIFTED)
            for (uint32_t i = 0; i < r.count; i++) D2D(keep.u() + (1 + r.first_slot + i) * n, coeff + (size_t)(r.d0 + i) * n, n);
}

static double host_ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

std::vector<uint8_t> Engine::export_saved(const Bundle &b, const u64 ntt_parms_id[4], uint32_t flags, int compr)
{
    Enter g(this);
    TIER1_SLOTS();
    lookup_check("export_saved");
    if (flags & ~(uint32_t)(SAVED_STRIPPED | SAVED_NO_CACHE)) throw std::invalid_argument("export_saved: unknown flag");
    const bool stripped = (flags & SAVED_STRIPPED) != 0, cache = !(flags & SAVED_NO_CACHE);
    if (stripped && !cache) throw std::invalid_argument("export_saved: a stripped BinBundle holds nothing but its cache, so STRIPPED and NO_CACHE together leave nothing to save");
    if (compr != sealio::COMPR_NONE && compr != sealio::COMPR_ZSTD) throw std::invalid_argument("export_saved: compr_mode is none (0) or zstd (2)");
    const size_t n = hp_.n;
    const uint32_t bins = psu_.bins_per_bundle, max_items = psu_.table_params.max_items_per_bin, degree = b.degree;
    // (unstripped, the same bound comes out of the bin counts below, with the bin's name)
    if (stripped && degree + 1 > max_items)
        throw std::invalid_argument("export_saved: the BinBundle has " + std::to_string(degree + 1) + " plaintexts, BinBundle::load accepts max_items_per_bin = " +
                                    std::to_string(max_items) + " at most");
    const BundleLayout y = layout_of(degree);
    OpClock &clk = clock_[OP_EXPORT];
    for (double &m : clk.ms) m = 0;
    // stamps: 0, 1 around decode and counts (bins_counted); 2, 3 around k_bins_rows; 4 in front of the root search, 5 behind it, 6
    // behind the multiplicities and their copies (bins_search)
    clk.evs.reserve(7);

    std::vector<u64> rows, row_off, bin_felts, bin_off;
    DevBuf keep;                                                       // a_0 and the a_{i h} in coefficient form mod t
    double copy_ms = 0;
    if (!stripped) {
        // bundle_bins' stages, and between them, while the columns of poly are whole, the bins' rows and the coefficient-form plaintexts
        // from the same decode
        const bool kernel = bins_prepare(b, BINS_FORM_AUTO);
        const uint32_t stride = std::max<uint32_t>(1, degree);
        std::vector<u64> roots(n * (size_t)stride);
        std::vector<uint32_t> counts(n);
        BinsCounted c{};
        BinsFound f;
        WITH_ARENA({
            f = BinsFound(); rows.clear(); row_off.clear(); copy_ms = 0;       // (the body runs again after an arena overflow)
            c = bins_counted(b, true, counts.data(), clk.evs);
            // a bin may hold max_items_per_bin - 1 items (receiver_db.cpp:388-389); build_bundle lets one more in, and its polynomial
            // of max_items_per_bin + 1 coefficients is what BinBundle::load's cache check refuses
            for (uint32_t s = 0; s < bins; s++)
                if (counts[s] != LOOKUP_NONE && counts[s] >= max_items)
                    throw std::invalid_argument("bin " + std::to_string(s) + " holds " + std::to_string(counts[s]) + " items: a saved BinBundle has at most max_items_per_bin - 1 = " +
                                                std::to_string(max_items - 1) + " per bin (BinBundle::load refuses the cache otherwise)");
            row_off = rows_offsets(counts.data(), bins, degree + 1);
            if (cache) {
                // BinBundle::load wants as many plaintexts as the longest matching polynomial has coefficients (bin_bundle.cpp:1356-1366): a
                // BinBundle uploaded with plaintexts above every bin's count has more
                uint32_t longest = 0;
                for (uint32_t s = 0; s < bins; s++) longest = std::max(longest, counts[s]);
                if (longest != degree)
                    throw std::invalid_argument("export_saved: the BinBundle has degree " + std::to_string(degree) + " but its longest bin holds " + std::to_string(longest) +
                                                " items: BinBundle::load refuses a cache whose plaintexts outnumber the longest matching polynomial's coefficients");
                const std::vector<int> tops = rows_tile_tops(counts.data(), n, bins);
                const u64 total = row_off.back();
                u64 *doff = ws(row_off.size()), *dout = ws(total + 1);
                int *dtops = ws_as<int>(tops.size());
                HIP_CHECK(hipMemcpyAsync(doff, row_off.data(), row_off.size() * sizeof(u64), hipMemcpyHostToDevice, st_));
                HIP_CHECK(hipMemcpyAsync(dtops, tops.data(), tops.size() * sizeof(int), hipMemcpyHostToDevice, st_));
                clk.evs.record(2, st_);
                launch_bins_rows(c.poly, n, degree + 1, c.dcounts, doff, dtops, bins, dout, st_);
                clk.evs.record(3, st_);
                keep_coeff_rows(b, c.coeff, keep);
                sync();
                const auto t0 = std::chrono::steady_clock::now();
                rows.resize(total);
                if (total) HIP_CHECK(hipMemcpy(rows.data(), dout, total * sizeof(u64), hipMemcpyDeviceToHost));   // one contiguous copy
                copy_ms = host_ms_since(t0);
            }
            clk.evs.record(4, st_);
            bins_search(c, kernel, &stride, clk.evs, 5, f);            // (divides the columns of poly)
            sync();
        });
        clk.ms[0] = clk.evs.ms(0, 1);
        clk.ms[1] = clk.evs.ms(4, 6);
        if (cache) clk.ms[2] = clk.evs.ms(2, 3);
        bins_finish(c, f, roots.data(), stride);
        bin_off.assign((size_t)bins + 1, 0);
        for (uint32_t s = 0; s < bins; s++) bin_off[s + 1] = bin_off[s] + counts[s];
        bin_felts.resize(bin_off[bins]);
        for (uint32_t s = 0; s < bins; s++) std::copy(roots.data() + (size_t)s * stride, roots.data() + (size_t)s * stride + counts[s], bin_felts.begin() + bin_off[s]);
    } else {
        // stripped: nothing but a_0 and the a_{i h} is decoded -- decode_bundle's steps up to the un-lift, on the H lifted slots alone
        const size_t H = b.use_ps ? b.H : 0;
        const int high = hp_.clamp_chain_idx(1);
        keep.alloc((H + 1) * n * sizeof(u64));
        D2D(keep.u(), b.a0.u(), n);
        if (H) {
            const size_t Lh = (size_t)high + 1, sb = b.packed ? b.lifted_slot_bytes : Lh * n * sizeof(u64);
            launch_limb0_rows(dlevel(high), (int)Lh, b.lifted.p(), sb, b.packed, keep.u() + n, n, H, st_);
            d_ntt(keep.u() + n, H, map_ct(), 1, true, data_primes_narrow_);
            launch_unlift(keep.u() + n, H * n, hp_.t, hp_.key_q[0], st_);
        }
        sync();
    }

    // the plaintexts, one degree at a time: the whole dense BinBundle is never on the host
    std::vector<std::vector<uint8_t>> blobs;
    double ser_ms = 0;
    if (cache) {
        const size_t Lpt = (size_t)b.pt_level + 1;
        blobs.resize((size_t)degree + 1);
        std::vector<u64> host(std::max(Lpt, (size_t)1) * n);
        DevBuf dense;
        if (b.packed && b.ntt_count) dense.alloc(Lpt * n * sizeof(u64));
        for (uint32_t d = 0; d <= degree; d++) {
            const BundleWhere w = y.where(d);
            const bool ntt = w.kind == COEFF_NTT;
            const size_t words = ntt ? Lpt * n : n;
            auto t0 = std::chrono::steady_clock::now();
            if (!ntt) HIP_CHECK(hipMemcpy(host.data(), keep.u() + (w.kind == COEFF_RAW ? 0 : 1 + w.slot) * n, words * sizeof(u64), hipMemcpyDeviceToHost));
            else if (b.packed) {
                launch_unpack_rows(dlevel(b.pt_level), (int)Lpt, static_cast<const char *>(b.ntt.p()) + w.slot * b.ntt_slot_bytes, b.ntt_slot_bytes, dense.u(), n, 1, st_);
                sync();
                HIP_CHECK(hipMemcpy(host.data(), dense.p(), words * sizeof(u64), hipMemcpyDeviceToHost));
            } else HIP_CHECK(hipMemcpy(host.data(), b.ntt.u() + w.slot * words, words * sizeof(u64), hipMemcpyDeviceToHost));
            copy_ms += host_ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            sealio::Plaintext pt;
            if (ntt) std::copy(ntt_parms_id, ntt_parms_id + 4, pt.parms_id);
            pt.coeff_count = words;
            pt.data.assign(host.begin(), host.begin() + words);
            blobs[d] = sealio::save_plaintext(pt, (uint8_t)compr);
            ser_ms += host_ms_since(t0);
        }
    }
    clk.ms[3] = copy_ms;
    clk.ms[4] = ser_ms;

    const auto t0 = std::chrono::steady_clock::now();
    wire::BinBundleParts parts;
    parts.bundle_idx = b.bundle_idx;
    parts.mod = hp_.t;
    parts.stripped = stripped;
    parts.has_cache = cache;
    parts.bin_felts = bin_felts.data(); parts.bin_off = bin_off.data(); parts.n_bins = stripped ? 0 : bins;
    parts.polyn_felts = rows.data(); parts.polyn_off = row_off.data(); parts.n_polyns = stripped || !cache ? 0 : bins;
    for (const auto &blob : blobs) parts.coeffs.push_back(wire::Span{ blob.data(), blob.size() });
    std::vector<uint8_t> out = wire::build_bin_bundle(parts);           // (refuses a buffer over the 32-bit limit before it allocates)
    clk.ms[5] = host_ms_since(t0);
    return out;
}

// ---- what a BinBundle answers in plaintext (bin_eval.h): decode, k_bin_counts, k_bins_eval, one BinBundle after the other through the
// workspace as the lookup runs them.  Queues only: inside the caller's WITH_ARENA, which syncs.  xs / masks: per BinBundle a device
// pointer to n slot values (masks, or an entry of it, may be null); out [n_bundles][n], is_bin [n_bundles][n] or null, bad: one zeroed
// word that a value >= t raises -- all device memory.  evs: the caller's stamps, reserved up to first + 4 n_bundles.
void Engine::eval_plain_queue(const Bundle *const *bundles, uint32_t n_bundles, const u64 *const *xs, const u64 *const *masks, u64 *out,
                              unsigned char *is_bin, u32 *bad, EventStamps &evs, size_t first)
{
    const size_t n = hp_.n;
    uint32_t *dcounts = ws_as<uint32_t>(n);
    const size_t mark = arena_off_;
    for (uint32_t i = 0; i < n_bundles; i++) {
        const Bundle &b = *bundles[i];
        arena_off_ = mark;                                             // one BinBundle after the other through the same workspace (stream order)
        evs.record(first + 4 * i, st_);
        const u64 *poly = decode_counted(b, dcounts, nullptr, &evs, first + 4 * i + 1);
        evs.record(first + 4 * i + 2, st_);
        launch_bins_eval(poly, n, b.degree + 1, dcounts, xs[i], masks ? masks[i] : nullptr, make_mod(hp_.t), out + (size_t)i * n,
                         is_bin ? is_bin + (size_t)i * n : nullptr, bad, st_);
        evs.record(first + 4 * i + 3, st_);
    }
}

// after the caller's sync
void Engine::eval_plain_collect(const EventStamps &evs, size_t first, uint32_t n_bundles, double *ms)
{
    ms[0] = ms[1] = ms[2] = 0;
    for (uint32_t i = 0; i < n_bundles; i++)
        for (int k = 0; k < 3; k++) ms[k] += evs.ms(first + 4 * i + k, first + 4 * i + k + 1);
}

static void check_slot_values(const u64 *v, size_t rows, size_t n, u64 t, const char *what)
{
    check_reduced(v, rows * n, t, [&](size_t i, u64 x) {
        return std::string(what) + " " + std::to_string(x) + " (row " + std::to_string(i / n) + ", slot " + std::to_string(i % n) + ")";
    });
}

void Engine::bundles_eval_plain(const Bundle *const *bundles, uint32_t n_bundles, const u64 *x, bool x_on_device, const u64 *masks, bool masks_on_device,
                                u64 *out, bool out_on_device, unsigned char *is_bin)
{
    Enter g(this);
    TIER1_SLOTS();
    lookup_check("eval_plain");
    if (!n_bundles) return;
    const size_t n = hp_.n, words = (size_t)n_bundles * n;
    if (!x_on_device) check_slot_values(x, n_bundles, n, hp_.t, "slot value");
    if (masks && !masks_on_device) check_slot_values(masks, n_bundles, n, hp_.t, "mask value");
    u32 bad_host = 0;
    OpClock &clk = clock_[OP_EVAL_PLAIN];
    clk.evs.reserve((size_t)4 * n_bundles);
    WITH_ARENA({
        const u64 *dx = x, *dm = masks;
        if (!x_on_device) {
            u64 *staged = ws(words);
            HIP_CHECK(hipMemcpyAsync(staged, x, words * sizeof(u64), hipMemcpyHostToDevice, st_));
            dx = staged;
        }
        if (masks && !masks_on_device) {
            u64 *staged = ws(words);
            HIP_CHECK(hipMemcpyAsync(staged, masks, words * sizeof(u64), hipMemcpyHostToDevice, st_));
            dm = staged;
        }
        u64 *dout = out_on_device ? out : ws(words);
        unsigned char *dbin = !is_bin ? nullptr : out_on_device ? is_bin : ws_as<unsigned char>(words);
        u32 *bad = ws_as<u32>(1, 1);
        HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(u64), st_));
        std::vector<const u64 *> xs(n_bundles), ms(n_bundles);
        for (uint32_t i = 0; i < n_bundles; i++) { xs[i] = dx + (size_t)i * n; ms[i] = dm ? dm + (size_t)i * n : nullptr; }
        eval_plain_queue(bundles, n_bundles, xs.data(), ms.data(), dout, dbin, bad, clk.evs, 0);
        if (!out_on_device) {
            HIP_CHECK(hipMemcpyAsync(out, dout, words * sizeof(u64), hipMemcpyDeviceToHost, st_));
            if (is_bin) HIP_CHECK(hipMemcpyAsync(is_bin, dbin, words, hipMemcpyDeviceToHost, st_));
        }
        HIP_CHECK(hipMemcpyAsync(&bad_host, bad, sizeof(u32), hipMemcpyDeviceToHost, st_));
        sync();
    });
    eval_plain_collect(clk.evs, 0, n_bundles, clk.ms);
    if (bad_host) throw std::invalid_argument(not_reduced("a slot or mask value on the device"));
}

// ---- the self-test (include/apsu_he.h: apsu_he_db_self_test): the querier's and the receiver's calls strung together on device buffers
// of this call, then the plaintext answer and the comparison.  The context's lock is taken per step, as by a caller who made these calls
// one by one; the BinBundles are only read.
SelfTestReport Engine::self_test(const Bundle *const *bundles, uint32_t count, const u64 seed[8], const u64 *x_host, const uint32_t *query_indices,
                                 uint32_t n_query, const uint32_t *mask_positions)
{
    SelfTestReport rep = self_test_empty();
    std::vector<uint32_t> idx;
    {
        Enter g(this);
        lookup_check("self_test");
        if (!hp_.using_keyswitching) throw std::invalid_argument("parameters do not support key switching: the reference creates no relinearisation keys");
        if (query_indices) idx.assign(query_indices, query_indices + n_query);
        else {
            for (uint32_t i = 0; i < count; i++) idx.push_back(bundles[i]->bundle_idx);
            std::sort(idx.begin(), idx.end());
            idx.erase(std::unique(idx.begin(), idx.end()), idx.end());
        }
        for (size_t k = 0; k < idx.size(); k++)
            if (idx[k] >= psu_.bundle_idx_count || (k && idx[k] <= idx[k - 1])) throw std::invalid_argument("bundle indices are ascending, distinct and in range");
        for (uint32_t i = 0; i < count; i++) {
            if (!std::binary_search(idx.begin(), idx.end(), bundles[i]->bundle_idx)) throw std::invalid_argument("a BinBundle's bundle index is not among the query's");
            if (mask_positions && mask_positions[i] >= SELF_TEST_MAX_OBJECTS) throw std::invalid_argument("too many BinBundles for one self-test");
        }
        if (count >= SELF_TEST_MAX_OBJECTS) throw std::invalid_argument("too many BinBundles for one self-test");
    }
    if (!count) return rep;
    const size_t n = hp_.n;
    const int K = hp_.K, L = hp_.first_chain_idx + 1, n_idx = (int)idx.size();
    const size_t S = psu_.query_params.query_powers.size();
    if (x_host) check_slot_values(x_host, idx.size(), n, hp_.t, "slot value");
    Blake2xbSeed sd;
    for (int i = 0; i < 8; i++) sd.w[i] = seed[i];
    auto pos = [&](uint32_t i) { return mask_positions ? mask_positions[i] : i; };
    // stamps: 0 behind the draws, 1 in front of the plaintext answer, 2 behind it, 3 behind the comparison; from 4 on eval_plain_queue's
    OpClock &clk = clock_[OP_SELF_TEST];

    DevBuf xs, mvals, menc, sk, cts, res, got, want;                   // allocated with the context's device current
    std::unique_ptr<RelinKeys> rk;
    std::unique_ptr<Powers> pw;
    // the key material of the call is overwritten before its buffers are released, whichever way the call ends: the secret key, the
    // relinearisation keys, and the workspace through which keygen and the key generation passed them
    auto wipe = [&] {
        try {
            Enter g(this);
            if (sk.bytes()) HIP_CHECK(hipMemsetAsync(sk.p(), 0, sk.bytes(), st_));
            if (rk && rk->data.bytes()) HIP_CHECK(hipMemsetAsync(rk->data.p(), 0, rk->data.bytes(), st_));
            if (arena_.bytes()) HIP_CHECK(hipMemsetAsync(arena_.p(), 0, arena_.bytes(), st_));
            sync();
        } catch (...) { }
    };
    try {
        {
            Enter g(this);
            clk.evs.reserve(4 + (size_t)4 * count);
            xs.alloc(idx.size() * n * sizeof(u64)); mvals.alloc((size_t)count * n * sizeof(u64)); menc.alloc((size_t)count * n * sizeof(u64));
            sk.alloc((size_t)K * n * sizeof(u64)); cts.alloc(idx.size() * S * 2 * L * n * sizeof(u64)); res.alloc((size_t)count * 2 * n * sizeof(u64));
            got.alloc((size_t)count * n * sizeof(u64)); want.alloc((size_t)count * n * sizeof(u64));
            if (x_host) HIP_CHECK(hipMemcpyAsync(xs.p(), x_host, xs.bytes(), hipMemcpyHostToDevice, st_));
            else launch_fill_blake2xb(xs.u(), idx.size() * n, sd, SELF_TEST_X_FIRST, hp_.t, st_);
            // the masks' slot values, position by position: the draws apsu_he_mask_generate_blake2xb encodes below
            for (uint32_t i = 0; i < count; i++) launch_fill_blake2xb(mvals.u() + (size_t)i * n, n, sd, SELF_TEST_MASK_FIRST + (u64)pos(i) * n, hp_.t, st_);
            clk.evs.record(0, st_);
        }
        keygen(seed, sk.u(), true);
        relin_keygen(sk.u(), seed, nullptr, nullptr, &rk, true);
        std::vector<u64> ct_seeds(idx.size() * S * 8);
        query_create(sk.u(), seed, idx.data(), n_idx, xs.u(), true, cts.u(), ct_seeds.data(), true);
        std::vector<const u64 *> src(idx.size() * S);
        for (size_t c = 0; c < src.size(); c++) src[c] = cts.u() + c * 2 * L * n;
        pw = compute_powers(idx.data(), n_idx, src.data(), true, rk.get());
        for (uint32_t i = 0; i < count;) {                             // runs of consecutive positions continue one stream
            uint32_t j = i + 1;
            while (j < count && pos(j) == pos(j - 1) + 1) j++;
            mask_generate_blake2xb(seed, SELF_TEST_MASK_FIRST + (u64)pos(i) * n, j - i, menc.u() + (size_t)i * n, nullptr, nullptr);
            i = j;
        }
        std::vector<const u64 *> mptr(count), xptr(count), vptr(count);
        for (uint32_t i = 0; i < count; i++) {
            mptr[i] = menc.u() + (size_t)i * n;
            vptr[i] = mvals.u() + (size_t)i * n;
            xptr[i] = xs.u() + (size_t)(std::lower_bound(idx.begin(), idx.end(), bundles[i]->bundle_idx) - idx.begin()) * n;
        }
        eval_bundles(bundles, (int)count, *pw, rk.get(), mptr.data(), true, res.u(), true);
        std::vector<int> budget(count);
        decrypt_decode(sk.u(), res.u(), true, count, nullptr, nullptr, budget.data(), true, got.u());
        u64 status[2] = { 0, EVAL_NO_MISMATCH };
        u32 bad_host = 0;
        {
            Enter g(this);
            TIER1_SLOTS();
            WITH_ARENA({
                clk.evs.record(1, st_);
                u64 *dstatus = ws(2);
                u32 *bad = ws_as<u32>(1, 1);
                const u64 init[2] = { 0, EVAL_NO_MISMATCH };
                HIP_CHECK(hipMemcpyAsync(dstatus, init, sizeof(init), hipMemcpyHostToDevice, st_));
                HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(u64), st_));
                eval_plain_queue(bundles, count, xptr.data(), vptr.data(), want.u(), nullptr, bad, clk.evs, 4);
                clk.evs.record(2, st_);
                launch_eval_compare(got.u(), want.u(), n, count, dstatus, st_);
                clk.evs.record(3, st_);
                HIP_CHECK(hipMemcpyAsync(status, dstatus, sizeof(status), hipMemcpyDeviceToHost, st_));
                HIP_CHECK(hipMemcpyAsync(&bad_host, bad, sizeof(u32), hipMemcpyDeviceToHost, st_));
                sync();
            });
            if (bad_host) throw std::logic_error(not_reduced("self_test: a drawn value"));
            rep.bundles = count;
            rep.slots = (u64)count * n;
            rep.mismatches = status[0];
            if (status[1] != EVAL_NO_MISMATCH) {
                rep.first_bundle = (int32_t)(status[1] >> 32);
                rep.first_slot = (uint32_t)status[1];
                const size_t at = (size_t)rep.first_bundle * n + rep.first_slot;
                HIP_CHECK(hipMemcpy(&rep.first_got, got.u() + at, sizeof(u64), hipMemcpyDeviceToHost));
                HIP_CHECK(hipMemcpy(&rep.first_expected, want.u() + at, sizeof(u64), hipMemcpyDeviceToHost));
            }
            for (uint32_t i = 0; i < count; i++)
                if (rep.min_budget_bundle < 0 || budget[i] < rep.min_budget_bits) { rep.min_budget_bits = budget[i]; rep.min_budget_bundle = (int32_t)i; }
            rep.he_ms = clk.evs.ms(0, 1);
            rep.plain_ms = clk.evs.ms(1, 3);
            eval_plain_collect(clk.evs, 4, count, clk.ms);
            clk.ms[3] = clk.evs.ms(2, 3);
            clk.ms[4] = rep.he_ms;
        }
    } catch (...) {
        wipe();
        if (pw) recycle_powers(std::move(pw));
        throw;
    }
    wipe();
    recycle_powers(std::move(pw));
    return rep;
}

} // namespace apsu_he
