// See engine.h.  Host orchestration of the HIP kernels; mirrors, step for step,
//   Receiver::ComputePowers                 receiver/apsu/receiver_osn.cpp:395-488
//   BatchedPlaintextPolyn::eval             receiver/apsu/bin_bundle.cpp:106-174
//   BatchedPlaintextPolyn::eval_patstock    receiver/apsu/bin_bundle.cpp:192-360
// Exact (rounding-free) steps are batched / re-associated freely; every rounding step
// (drop-limb, BEHZ floor, key-switch mod-down) is applied per term exactly where the reference
// applies it (SURVEY.md §2.4 note N1), so results are bit-identical to the CPU path.
#include "engine_impl.h"
#include "sched_policy.h"
#include "seal_codec.h"

#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

namespace apsu_he {

void throw_hip(hipError_t e, const char *file, int line)
{
    throw HipError(std::string("HIP error: ") + hipGetErrorString(e) + " at " + file + ":" + std::to_string(line));
}

void DevBuf::alloc(size_t bytes)
{
    release();
    if (!bytes) return;
    HIP_CHECK(hipMalloc(&p_, bytes));
    bytes_ = bytes;
}
void DevBuf::release()
{
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    bytes_ = 0;
}

int Powers::slot_of(uint32_t bundle_idx) const
{
    for (int i = 0; i < nb; i++) if (bundle_indices[i] == bundle_idx) return i;
    return -1;
}

// ============================================================================ construction
Engine::Engine(const HeParams &hp, const PSUParams *psu, int device) : hp_(hp), device_(device)
{
    if (psu) { psu_ = *psu; has_psu_ = true; }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        throw HipError("no HIP device available: the query-evaluation engine has no CPU fallback");
    if (device < 0 || device >= ndev) throw std::invalid_argument("device index out of range");
    DeviceConstants dc = build_device_constants(hp_);            // (refuses ring sizes and limb counts the kernels do not have)
    data_primes_narrow_ = dc.data_primes_narrow;
    ext_primes_narrow_ = dc.ext_primes_narrow;
    unlift_exact_ = dc.unlift_exact;
    key_level_ = dc.key_level;
    max_multiple_ = dc.max_multiple;
    if (hp_.logn == 15) fuse_tensor_ = false;                    // the fused load belongs to a whole-limb workgroup
    packed_rows_ = sw_.packed_rows && hp_.using_keyswitching;    // (the single-prime paths keep dense rows)
    struct Restore { int prev = -1; ~Restore() { if (prev >= 0) (void)hipSetDevice(prev); } } restore;
    { int cur = -1; if (hipGetDevice(&cur) == hipSuccess && cur != device) restore.prev = cur; }
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
    {   // the second stream carries short latency-bound chains that must make progress next to a grid-filling kernel
        // of the main stream (the BinBundle inner products): highest dispatch priority
        int least = 0, greatest = 0;
        HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_CHECK(hipStreamCreateWithPriority(&lanes_[1].st, hipStreamNonBlocking, greatest));
        HIP_CHECK(hipStreamCreateWithPriority(&lanes_[2].st, hipStreamNonBlocking, greatest));
    }
    HIP_CHECK(hipEventCreateWithFlags(&ev_main_, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&ev_side_, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&ev_intt_, hipEventDisableTiming));

    // Every constant the kernels read comes from build_device_constants (dev_consts.cpp).  One allocation per table, in this order:
    // order and sizes are part of the allocator state the database upload meets (k_mac's rate depends on where the
    // later buffers land).  Then the tables' addresses go into the structs that name them, then everything is uploaded.
    auto each = [&](auto f) {
        f(d_tw_, dc.tw); f(d_tabs_, dc.tabs); f(d_fin_, dc.fin); f(d_drop_, dc.drop); f(d_levels_, dc.levels);
        f(d_map_ext_, dc.map_ext); f(d_map_ext_fin_, dc.map_ext_fin); f(d_map_ks_, dc.map_ks); f(d_map_ksacc_, dc.map_ksacc);
        f(d_map_ksacc_raw_, dc.map_ksacc_raw); f(d_map_ct_, dc.map_ct); f(d_mdtw_, dc.mdtw);
    };
    each([](DevBuf &b, const auto &v) { b.alloc(v.size() * sizeof(v[0])); });
    d_key_.alloc(sizeof(DevKey));
    dc.relocate(reinterpret_cast<const TwPair *>(d_tw_.p()), reinterpret_cast<const ShoupConst *>(d_fin_.p()),
                reinterpret_cast<const ShoupConst *>(d_drop_.p()), reinterpret_cast<const ShoupConst *>(d_mdtw_.p()));
    each([](DevBuf &b, const auto &v) { if (b.p()) HIP_CHECK(hipMemcpy(b.p(), v.data(), b.bytes(), hipMemcpyHostToDevice)); });
    HIP_CHECK(hipMemcpy(d_key_.p(), &dc.key, sizeof(DevKey), hipMemcpyHostToDevice));
    if (hp_.batching) {
        d_slot_map_.alloc(hp_.slot_map.size() * sizeof(uint32_t));
        HIP_CHECK(hipMemcpy(d_slot_map_.p(), hp_.slot_map.data(), hp_.slot_map.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (has_psu_) {
        auto targets = create_powers_set(psu_.query_params.ps_low_degree, psu_.table_params.max_items_per_bin);
        if (!dag_.configure(psu_.query_params.query_powers, targets))
            throw std::invalid_argument("failed to configure PowersDag");
        build_schedule();
        // polynomials per target power: 2 with key switching; without it a product has size(parent1) + size(parent2) - 1
        const uint32_t max_power = *dag_.target_powers().rbegin();
        nks_size_.assign(max_power + 1, 0);
        for (uint32_t p : dag_.target_powers()) nks_size_[p] = 2;
        nks_ = !hp_.using_keyswitching && dag_.depth() > 0;
        if (nks_) {
            uint32_t widest = 2;
            for (const auto &nd : sched_.nodes) {                 // slot order: parents come first
                const uint32_t a = nks_size_[sched_.slot_power[nd[1]]], b = nks_size_[sched_.slot_power[nd[2]]];
                const uint32_t sz = std::min<uint32_t>(a + b - 1, 2 * CT_SIZE_MAX);        // (kept finite; anything above the limit throws)
                nks_size_[sched_.slot_power[nd[0]]] = sz;
                widest = std::max(widest, sz);
            }
            nks_oversize_ = widest > CT_SIZE_MAX;
            nks_S_ = (std::min(widest, CT_SIZE_MAX) + 1) & ~1u;
        }
        if (!hp_.using_keyswitching)                              // (eval_patstock alone already leaves three polynomials)
            for (uint32_t deg = 0; deg <= psu_.table_params.max_items_per_bin; deg++) {
                const uint32_t r = result_size_for(deg);
                if (r <= CT_SIZE_MAX) result_polys_ = std::max(result_polys_, r);
            }
    }
    const size_t init = sw_.arena_bytes != EngineSwitches::ARENA_AUTO ? sw_.arena_bytes : 4096 * hp_.n * sizeof(u64);   // 256 MiB at n = 8192; grows on demand
    arena_.alloc(init);
    lanes_[1].arena.alloc(std::max<size_t>(init / 4, (size_t)1 << 20));
    lanes_[2].arena.alloc((size_t)1 << 20);
    stage_bytes_ = 4u << 20;
    HIP_CHECK(hipHostMalloc(&stage_, stage_bytes_));
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&bad_source_), BAD_SLOTS * sizeof(unsigned)));
    for (int i = 0; i < BAD_SLOTS; i++) bad_source_[i] = 0;
}

Engine::~Engine()
{
    int cur = -1;
    const bool switched = hipGetDevice(&cur) == hipSuccess && cur != device_ && hipSetDevice(device_) == hipSuccess;
    struct Back { bool on; int dev; ~Back() { if (on) (void)hipSetDevice(dev); } } back{ switched, cur };
    // queued work first (apsu_he_set_async_results leaves evaluations in flight), then the buffers it uses
    if (st_) (void)hipStreamSynchronize(st_);
    for (Lane &l : lanes_) if (l.st) (void)hipStreamSynchronize(l.st);
    powers_pool_.clear();
    if (st_) (void)hipStreamDestroy(st_);
    for (Lane &l : lanes_) if (l.st) (void)hipStreamDestroy(l.st);
    for (hipEvent_t e : inflight_) if (e) (void)hipEventDestroy(e);
    for (PhaseSpan &sp : phase_spans_) for (hipEvent_t e : { sp.a, sp.b, sp.b2 }) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : phase_pool_) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : { query_start_, query_end_ }) if (e) (void)hipEventDestroy(e);
    if (ev_main_) (void)hipEventDestroy(ev_main_);
    for (OpClock &c : clock_) c.evs.release();
    if (ev_fork_) (void)hipEventDestroy(ev_fork_);
    if (ev_side_) (void)hipEventDestroy(ev_side_);
    if (ev_intt_) (void)hipEventDestroy(ev_intt_);
    if (stage_) (void)hipHostFree(stage_);
    if (bad_source_) (void)hipHostFree(bad_source_);
    if (wire_pinned_) (void)hipHostFree(wire_pinned_);
}

void Engine::wire_stage(size_t bytes, u64 **device, u64 **pinned)
{
    Enter g(this);                                               // (device guard; the buffers belong to this engine's device)
    if (wire_dev_.bytes() < bytes) { sync(); wire_dev_.alloc(bytes + bytes / 4); }
    if (wire_pinned_bytes_ < bytes) {
        sync();
        if (wire_pinned_) (void)hipHostFree(wire_pinned_);
        wire_pinned_ = nullptr; wire_pinned_bytes_ = 0;
        HIP_CHECK(hipHostMalloc(&wire_pinned_, bytes + bytes / 4));
        wire_pinned_bytes_ = bytes + bytes / 4;
    }
    *device = wire_dev_.u();
    *pinned = static_cast<u64 *>(wire_pinned_);
}

void Engine::sync()
{
    counters_[C_HOST_SYNC]++;
    HIP_CHECK(hipStreamSynchronize(st_));
    for (Lane &l : lanes_) if (l.st) HIP_CHECK(hipStreamSynchronize(l.st));
    if (prof_on_) prof_collect();
}

// Called where a PUBLIC entry point has just waited for the device (apsu_he_sync, a synchronous apsu_he_eval_bundles, apsu_he_powers_download):
// k_copy_sources of a query whose work has completed by now may have found a source coefficient outside [0, q).  (Not inside sync():
// the engine also waits in the middle of its own bookkeeping -- arena growth, job-table reallocation -- where nothing may be thrown.)
bool Engine::bad_source_pending(int slot, bool take)
{
    if (!bad_source_) return false;
    const unsigned v = *const_cast<volatile unsigned *>(bad_source_ + slot);
    if (v == bad_reported_[slot]) return false;
    if (take) bad_reported_[slot] = v;
    return true;
}

static const char *const BAD_SOURCE_TEXT = "a source ciphertext of apsu_he_compute_powers holds a coefficient outside [0, q): the results computed from it "
                                           "are not valid (seal::is_data_valid_for)";

void Engine::check_sources()
{
    bool any = false;
    for (int i = 0; i < BAD_SLOTS; i++) any |= bad_source_pending(i, true);
    if (any) throw std::invalid_argument(BAD_SOURCE_TEXT);
}

// the report of ONE query: only the word its ComputePowers writes, and only that call's sequence number in it (an older or a newer
// query's report stays where it is for the call that waits for that query, or for apsu_he_sync)
void Engine::check_sources(const Powers &pw)
{
    const int slot = (int)(pw.seq % BAD_SLOTS);
    if (!bad_source_ || !pw.seq) return;
    const unsigned v = *const_cast<volatile unsigned *>(bad_source_ + slot);
    if (v == pw.seq && bad_reported_[slot] != v) {
        bad_reported_[slot] = v;
        throw std::invalid_argument(BAD_SOURCE_TEXT);
    }
}

bool Engine::take_bad_source()
{
    Enter g(this);
    bool any = false;
    for (int i = 0; i < BAD_SLOTS; i++) any |= bad_source_pending(i, true);
    return any;
}

void Engine::wait()
{
    Enter g(this);
    sync();
    check_sources();
}

void Engine::drain()
{
    Enter g(this);
    sync();
}

void Engine::switch_lane(int lane)
{
    if (lane == cur_lane_) return;
    for (Lane *l : { &lanes_[cur_lane_], &lanes_[lane] }) {      // park the current lane in its (empty) place, take the other one out of its
        std::swap(st_, l->st);
        std::swap(arena_, l->arena);
        std::swap(arena_off_, l->off);
        std::swap(job_seq_, l->job_seq);
    }
    cur_lane_ = lane;
}

// ---- profiling: one HIP event pair per launch on the engine's stream, resolved at the next sync
void Engine::profile_enable(int mode)
{
    Enter g(this);
    HIP_CHECK(hipStreamSynchronize(st_));
    for (Lane &l : lanes_) if (l.st) HIP_CHECK(hipStreamSynchronize(l.st));
    prof_collect();
    prof_on_ = mode != 0;
    prof_ntt_only_ = mode == 2;
}

void Engine::profile_read(ProfStats *out, bool reset)
{
    Enter g(this);
    HIP_CHECK(hipStreamSynchronize(st_));
    for (Lane &l : lanes_) if (l.st) HIP_CHECK(hipStreamSynchronize(l.st));
    prof_collect();
    if (out) *out = prof_;
    if (reset) prof_ = ProfStats{};
}

void Engine::prof_begin(int kind, uint64_t units)
{
    if (!prof_on_ || (prof_ntt_only_ && kind > P_NTT_INV && kind != P_NTT_FUSED)) return;
    ProfRec r{ nullptr, nullptr, kind, units };
    for (hipEvent_t *e : { &r.a, &r.b }) {
        if (!prof_pool_.empty()) { *e = prof_pool_.back(); prof_pool_.pop_back(); }
        else HIP_CHECK(hipEventCreate(e));
    }
    HIP_CHECK(hipEventRecord(r.a, st_));
    prof_recs_.push_back(r);
    prof_open_ = true;
}

void Engine::prof_end()
{
    if (!prof_open_ || prof_recs_.empty()) return;
    HIP_CHECK(hipEventRecord(prof_recs_.back().b, st_));
    prof_open_ = false;
}

void Engine::prof_collect()
{
    // a sync can happen inside an open scope (job-buffer growth): keep that record for later
    ProfRec open_rec{};
    const bool keep = prof_open_ && !prof_recs_.empty();
    if (keep) { open_rec = prof_recs_.back(); prof_recs_.pop_back(); }
    for (auto &r : prof_recs_) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            prof_.ms[r.kind] += ms;
            prof_.launches[r.kind] += 1;
            prof_.units[r.kind] += r.units;
        }
        prof_pool_.push_back(r.a);
        prof_pool_.push_back(r.b);
    }
    prof_recs_.clear();
    if (keep) prof_recs_.push_back(open_rec);
}

// ---- phase timers
const char *Engine::phase_name(int phase)
{
    static const char *names[PH_COUNT] = { "Receiver::RunQuery", "Receiver::ComputePowers", "Receiver::ProcessBinBundleCache" };
    return phase >= 0 && phase < PH_COUNT ? names[phase] : "";
}

hipEvent_t Engine::phase_event(hipStream_t st)
{
    hipEvent_t e = nullptr;
    if (!phase_pool_.empty()) { e = phase_pool_.back(); phase_pool_.pop_back(); }
    else HIP_CHECK(hipEventCreate(&e));
    HIP_CHECK(hipEventRecord(e, st));
    return e;
}

void Engine::phase_close_query()
{
    if (query_start_ && query_end_) phase_spans_.push_back(PhaseSpan{ query_start_, query_end_, nullptr, PH_RUN_QUERY });
    else { if (query_start_) phase_pool_.push_back(query_start_); if (query_end_) phase_pool_.push_back(query_end_); }
    query_start_ = query_end_ = nullptr;
}

void Engine::phase_collect()
{
    for (PhaseSpan &sp : phase_spans_) {
        float ms = 0, ms2 = 0;
        if (hipEventSynchronize(sp.b) == hipSuccess && hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess) {
            if (sp.b2 && hipEventSynchronize(sp.b2) == hipSuccess && hipEventElapsedTime(&ms2, sp.a, sp.b2) == hipSuccess) ms = std::max(ms, ms2);
            PhaseSummary &p = phase_[sp.phase];
            p.min_ms = p.count ? std::min(p.min_ms, (double)ms) : ms;
            p.max_ms = p.count ? std::max(p.max_ms, (double)ms) : ms;
            p.sum_ms += ms;
            p.count++;
        }
        for (hipEvent_t e : { sp.a, sp.b, sp.b2 }) if (e) phase_pool_.push_back(e);
    }
    phase_spans_.clear();
}

void Engine::phase_enable(bool on)
{
    Enter g(this);
    if (!on && phase_on_) { phase_close_query(); phase_collect(); }
    phase_on_ = on;
}

void Engine::phase_read(PhaseSummary *out, bool reset)
{
    Enter g(this);
    phase_close_query();
    phase_collect();
    if (out) for (int i = 0; i < PH_COUNT; i++) out[i] = phase_[i];
    if (reset) for (int i = 0; i < PH_COUNT; i++) phase_[i] = PhaseSummary{};
}

// where slot `slot` of a BinBundle's NTT-form plaintexts (lifted = false) or of its pre-lifted coefficient-form ones starts, and the
// distance between consecutive slots in the unit k_mac takes it in (words for dense rows, BYTES for bit-packed ones)
static const u64 *bundle_slot(const Bundle &b, bool lifted, size_t slot, size_t dense_words)
{
    const DevBuf &buf = lifted ? b.lifted : b.ntt;
    if (!b.packed) return buf.u() + slot * dense_words;
    return reinterpret_cast<const u64 *>(static_cast<const char *>(buf.p()) + slot * (lifted ? b.lifted_slot_bytes : b.ntt_slot_bytes));
}
static u32 bundle_stride(const Bundle &b, bool lifted, size_t dense_words)
{
    return b.packed ? (u32)(lifted ? b.lifted_slot_bytes : b.ntt_slot_bytes) : (u32)dense_words;
}
void Engine::check_level(int chain_idx) const
{
    if (chain_idx < 0 || chain_idx > hp_.first_chain_idx) throw std::invalid_argument("chain_idx is not a data level");
}

// seal::is_data_valid_for on tier-1 ciphertext data: the kernels take canonical residues (the product-free inverse butterflies
// wrap mod 2^64 on a word >= q, the lazy loaders bound their sums by q), so a word outside [0, q_j) is refused rather than turned
// into a silently wrong limb.  Device operands (apsu_he_set_tier1_on_device) are not read back: keeping them canonical is the
// caller's precondition (include/apsu_he.h).
void Engine::check_tier1_residues(const u64 *ct, size_t polys, int chain_idx, const char *what) const
{
    if (tier1_device_) return;
    const size_t n = hp_.n, L = (size_t)chain_idx + 1;
    for (size_t p = 0; p < polys; p++)
        for (size_t j = 0; j < L; j++) {
            const u64 *row = ct + (p * L + j) * n, qj = hp_.key_q[j];
            u64 bad = 0;
            for (size_t k = 0; k < n; k++) bad |= (u64)(row[k] >= qj);
            if (bad) throw std::invalid_argument(what);
        }
}

// ============================================================================ arena
u64 *Engine::ws(size_t words)
{
    size_t bytes = (words * sizeof(u64) + 255) & ~(size_t)255;
    if (arena_off_ + bytes > arena_.bytes()) { overflow_lane_ = cur_lane_; throw ArenaOverflow{ arena_off_ + bytes }; }
    u64 *p = reinterpret_cast<u64 *>(static_cast<char *>(arena_.p()) + arena_off_);
    arena_off_ += bytes;
    return p;
}

void Engine::ws_reset(size_t need)
{
    if (need) {                                   // grow the lane whose bump allocator overflowed
        switch_lane(overflow_lane_);
        if (need > arena_.bytes()) {
            counters_[C_ARENA_GROW]++;
            sync();
            arena_.release();
            arena_.alloc(need + need / 4);
        }
    }
    switch_lane(0);
    arena_off_ = 0;
    job_seq_ = job_seq_base_;
    lanes_[1].off = 0;
    lanes_[1].job_seq = job_seq_base_ + 128;      // lane 1 uses the upper half of the call's job-cache slots,
    lanes_[2].off = 0;
    lanes_[2].job_seq = job_seq_base_ + 240;      // lane 2 (a handful of tables) its last sixteen
}

template <class T> const T *Engine::upload_jobs(const std::vector<T> &v)
{
    if (v.empty()) return nullptr;
    const size_t bytes = v.size() * sizeof(T);
    // lanes 1 and 2 run next to other lanes' kernels: their tables must stay inside their own slot ranges (ws_reset; a pipelined
    // ComputePowers uses 12 of lane 1's 112)
    if ((cur_lane_ == 1 && job_seq_ >= job_seq_base_ + 240) || (cur_lane_ == 2 && job_seq_ >= job_seq_base_ + 256))
        throw std::logic_error("job-table slots of a side lane exhausted");
    if (job_seq_ >= job_slots_.size()) job_slots_.resize(job_seq_ + 1);
    JobSlot &slot = job_slots_[job_seq_++];
    for (JobWay &w : slot.way)
        if (w.host.size() == bytes && std::memcmp(w.host.data(), v.data(), bytes) == 0) {
            counters_[C_JOB_HIT]++;
            w.stamp = ++job_stamp_;
            return reinterpret_cast<const T *>(w.buf.p());                                            // unchanged since an earlier call
        }
    counters_[C_JOB_UPLOAD]++;
    JobWay *lru = &slot.way[0];
    for (JobWay &w : slot.way) if (w.stamp < lru->stamp) lru = &w;                                    // least recently used
    JobWay &way = *lru;
    way.stamp = ++job_stamp_;
    if (way.buf.bytes() < bytes) {
        counters_[C_JOB_REALLOC]++;
        sync();                                   // the old buffer may still be read by queued kernels
        way.buf.alloc(bytes + bytes / 2);
    }
    // through a pinned staging area so the copy is truly asynchronous and the std::vector may die
    const size_t aligned = (bytes + 63) & ~(size_t)63;
    if (stage_off_ + aligned > stage_bytes_) {
        counters_[C_STAGE_WRAP]++;
        sync();                                   // everything staged so far has been consumed
        if (aligned > stage_bytes_) {
            if (stage_) (void)hipHostFree(stage_);
            stage_bytes_ = aligned * 2;
            HIP_CHECK(hipHostMalloc(&stage_, stage_bytes_));
        }
        stage_off_ = 0;
    }
    char *hp = static_cast<char *>(stage_) + stage_off_;
    std::memcpy(hp, v.data(), bytes);
    stage_off_ += aligned;
    HIP_CHECK(hipMemcpyAsync(way.buf.p(), hp, bytes, hipMemcpyHostToDevice, st_));
    way.host.assign(reinterpret_cast<const unsigned char *>(v.data()), reinterpret_cast<const unsigned char *>(v.data()) + bytes);
    return reinterpret_cast<const T *>(way.buf.p());
}

void Engine::throttle_inflight()
{
    while (inflight_count_ >= (size_t)std::max(1, max_inflight_)) {
        HIP_CHECK(hipEventSynchronize(inflight_[inflight_head_]));
        inflight_head_ = (inflight_head_ + 1) % inflight_.size();
        inflight_count_--;
    }
}

void Engine::mark_inflight()
{
    const size_t cap = (size_t)std::max(1, max_inflight_) + 1;
    if (inflight_.size() != cap) {                               // (re)build the ring; nothing pending survives a resize
        for (size_t i = 0; i < inflight_count_; i++) (void)hipEventSynchronize(inflight_[(inflight_head_ + i) % inflight_.size()]);
        for (hipEvent_t e : inflight_) (void)hipEventDestroy(e);
        inflight_.assign(cap, nullptr);
        for (hipEvent_t &e : inflight_) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        inflight_head_ = inflight_count_ = 0;
    }
    throttle_inflight();
    const size_t at = (inflight_head_ + inflight_count_) % inflight_.size();
    HIP_CHECK(hipEventRecord(inflight_[at], st_));
    inflight_count_++;
}

void Engine::recycle_powers(std::unique_ptr<Powers> p)
{
    Enter g(this);
    if (!p) return;
    // keep the most recently released buffers: a context that changes its batch shape must not be left with a pool
    // full of buffers of the old shape (every call would then allocate and free ~100 MB)
    if (powers_pool_.size() >= 6) powers_pool_.erase(powers_pool_.begin());
    powers_pool_.push_back(std::move(p));
}

// ============================================================================ device building blocks
// the multiply-accumulate launch of `streams` over the first nlimbs primes: planned (mac_plan.h: jobs, form, grid) ...
MacPlan Engine::plan_mac(const std::vector<MacStream> &streams, size_t nlimbs, size_t n) const { return mac_plan(streams, hp_.key_q.data(), (int)nlimbs, n, sw_.mac_kara); }
// ... and launched on the current stream (jobs: the plan's jobs where they were uploaded earlier, ps_tables)
void Engine::d_mac(const MacPlan &p, const MacJob *jobs)
{
    PROF(P_MAC, p.units);
    launch_mac(dlevel(p.nlimbs - 1), p.nlimbs, jobs ? jobs : upload_jobs(p.jobs), p.n, (int)p.jobs.size(), st_, p.kara, p.packed, p.grid);
}

void Engine::d_ntt(u64 *data, size_t count, const int *modmap, int period, bool inverse, bool narrow)
{
    PROF(inverse ? P_NTT_INV : P_NTT_FWD, count);
    launch_ntt(hp_.logn, inverse, data, count, tabs(), modmap, period, st_, sw_.ntt_latency_limbs, narrow);
}

bool Engine::d_relinearize(u64 *ct3, size_t ct_stride, int batch, const RelinKeys &rk, int chain_idx, u64 *ext_out, int n_ext, u64 **defer_moddown)
{
    const int L = chain_idx + 1;
    const size_t n = hp_.n;
    u64 *tdec = ws((size_t)batch * (L + 1) * L * n);
    {   // tdec[b][I][J] = NTT_I(c2[b][J] mod m_I): the decomposition is the NTT's load (no separate pass)
        std::vector<const u64 *> src((size_t)batch * (L + 1) * L);
        for (int b = 0; b < batch; b++)
            for (int I = 0; I <= L; I++)
                for (int J = 0; J < L; J++) src[((size_t)b * (L + 1) + I) * L + J] = ct3 + (size_t)b * ct_stride + ((size_t)2 * L + J) * n;
        // sources are residues of q_0 .. q_{L-1}, targets q_0 .. q_{L-1} and the special prime: with SEAL's narrow coefficient primes
        // the lazy transform takes them as they are (16M-4096: 56-bit sources into 56- and 50-bit targets)
        u64 max_src = 0;
        for (int J = 0; J < L; J++) max_src = std::max(max_src, hp_.key_q[J]);
        bool nored = hp_.logn <= 14;
        for (int I = 0; I <= L && nored; I++) nored = ntt_gather_nored_ok(hp_.key_q[I < L ? I : hp_.K - 1], max_src, hp_.logn);
        PROF(P_NTT_FWD, src.size());
        launch_ntt_gather(hp_.logn, upload_jobs(src), tdec, src.size(), tabs(), map_ks(chain_idx), (L + 1) * L, st_, nored, sw_.ntt_latency_limbs, data_primes_narrow_);
    }
    u64 *acc = ws((size_t)batch * 2 * (L + 1) * n);
    // the inverse transform leaves its twist to the mod-down kernel, whose own constants absorb it (unrolled sizes)
    const bool raw = L <= 4;
    const int *amap = raw ? map_ksacc_raw(chain_idx) : map_ksacc(chain_idx);
    // (the inner product formed by the inverse transform's load, the way the BEHZ tensor product is, was measured in round 3:
    //  2 % SLOWER on the whole query -- six operand streams per output and tdec read twice; tools/microbench/intt_ks_experiment.hip)
    { PROFW(P_KEYSWITCH, (size_t)batch * n * ((size_t)L * (L + 1) + 2 * (L + 1))); launch_ks_inner(dkey(), L, tdec, rk.data.u(), acc, n, batch, st_); }
    d_ntt(acc, (size_t)batch * 2 * (L + 1), amap, L + 1, true, false);
    if (defer_moddown) {
        *defer_moddown = raw ? acc : nullptr;
        if (raw) return false;                                   // the caller's epilogue kernel takes it from here
    }
    const bool fuse_ext = ext_out && n_ext > 0 && hlevel(chain_idx).L == hlevel(chain_idx).nB && L <= 3;
    { PROFW(P_KEYSWITCH, (size_t)batch * n * (2 * (L + 1) + 4 * L) + (fuse_ext ? (size_t)n_ext * 2 * (hlevel(chain_idx).L + hlevel(chain_idx).nB + 1) * n : 0));
      launch_ks_moddown(dkey(), L, acc, ct3, ct_stride, n, batch, st_, dlevel(chain_idx), fuse_ext ? ext_out : nullptr, fuse_ext ? n_ext : 0, raw); }
    return fuse_ext;
}

// ============================================================================ tier 1
void Engine::transform_to_ntt(u64 *ct, int polys, int chain_idx)
{
    Enter g(this);
    TIER1_SLOTS();
    check_level(chain_idx);
    check_tier1_residues(ct, polys, chain_idx, "transform_to_ntt: operand holds a coefficient outside [0, q)");
    const size_t w = (size_t)polys * (chain_idx + 1) * hp_.n;
    WITH_ARENA({
        u64 *d = ws(w);
        H2D(d, ct, w);
        d_ntt_ct(d, polys, chain_idx, false);
        D2H(ct, d, w);
        tier1_done();
    });
}

void Engine::transform_from_ntt(u64 *ct, int polys, int chain_idx)
{
    Enter g(this);
    TIER1_SLOTS();
    check_level(chain_idx);
    check_tier1_residues(ct, polys, chain_idx, "transform_from_ntt: operand holds a coefficient outside [0, q)");
    const size_t w = (size_t)polys * (chain_idx + 1) * hp_.n;
    WITH_ARENA({
        u64 *d = ws(w);
        H2D(d, ct, w);
        d_ntt_ct(d, polys, chain_idx, true);
        D2H(ct, d, w);
        tier1_done();
    });
}

void Engine::multiply_plain_ntt(const u64 *ct, const u64 *pt_ntt, u64 *out, int polys, int chain_idx)
{
    Enter g(this);
    TIER1_SLOTS();
    check_level(chain_idx);
    check_tier1_residues(ct, polys, chain_idx, "multiply_plain_ntt: operand holds a coefficient outside [0, q)");
    check_tier1_residues(pt_ntt, 1, chain_idx, "multiply_plain_ntt: NTT-form plaintext holds a coefficient outside [0, q)");
    const size_t n = hp_.n, L = chain_idx + 1, w = polys * L * n;
    WITH_ARENA({
        u64 *d = ws(w), *p = ws(L * n), *o = ws(w);
        H2D(d, ct, w);
        H2D(p, pt_ntt, L * n);
        launch_dyadic_plain(dlevel(chain_idx), d, p, o, polys, n, 1, 0, st_);
        D2H(out, o, w);
        tier1_done();
    });
}

void Engine::transform_plain_to_ntt(const u64 *pt, size_t pt_coeffs, u64 *out, int chain_idx)
{
    Enter g(this);
    TIER1_SLOTS();
    check_level(chain_idx);
    const size_t n = hp_.n, L = chain_idx + 1;
    if (pt_coeffs > n) throw std::invalid_argument("plaintext has too many coefficients");
    WITH_ARENA({
        u64 *p = ws(n), *o = ws(L * n);
        HIP_CHECK(hipMemsetAsync(p, 0, n * sizeof(u64), st_));
        H2D(p, pt, pt_coeffs);
        launch_lift(dlevel(chain_idx), p, o, n, 1, nullptr, st_);
        d_ntt_ct(o, 1, chain_idx, false);
        D2H(out, o, L * n);
        tier1_done();
    });
}

// multiply_plain on coefficient-form ct and plaintext (bin_bundle.cpp:334): lift, NTT both,
// dyadic product, INTT.  SEAL's monomial shortcut (no lift) is honoured.
void Engine::multiply_plain(const u64 *ct, const u64 *pt, size_t pt_coeffs, u64 *out, int polys, int chain_idx)
{
    Enter g(this);
    TIER1_SLOTS();
    check_level(chain_idx);
    check_tier1_residues(ct, polys, chain_idx, "multiply_plain: operand holds a coefficient outside [0, q)");
    const size_t n = hp_.n, L = chain_idx + 1, w = polys * L * n;
    if (pt_coeffs > n) throw std::invalid_argument("plaintext has too many coefficients");
    const unsigned char mono = !tier1_device_ && is_monomial(pt, pt_coeffs) ? 1 : 0;      // (device operands: flagged by a kernel below)
    WITH_ARENA({
        u64 *d = ws(w), *p = ws(n), *pl = ws(L * n), *o = ws(w), *flag = ws(1);
        H2D(d, ct, w);
        HIP_CHECK(hipMemsetAsync(p, 0, n * sizeof(u64), st_));
        H2D(p, pt, pt_coeffs);
        if (tier1_device_) launch_flag_monomial(p, n, 1, reinterpret_cast<unsigned char *>(flag), st_);
        else HIP_CHECK(hipMemcpyAsync(flag, &mono, 1, hipMemcpyHostToDevice, st_));
        launch_lift(dlevel(chain_idx), p, pl, n, 1, reinterpret_cast<const unsigned char *>(flag), st_);
        d_ntt_ct(pl, 1, chain_idx, false);
        d_ntt_ct(d, polys, chain_idx, false);
        launch_dyadic_plain(dlevel(chain_idx), d, pl, o, polys, n, 1, 0, st_);
        d_ntt_ct(o, polys, chain_idx, true);
        D2H(out, o, w);
        tier1_done();
    });
}

void Engine::add(u64 *acc, const u64 *x, int polys, int chain_idx)
{
    Enter g(this);
    TIER1_SLOTS();
    check_level(chain_idx);
    check_tier1_residues(acc, polys, chain_idx, "add: operand holds a coefficient outside [0, q)");
    check_tier1_residues(x, polys, chain_idx, "add: operand holds a coefficient outside [0, q)");
    const size_t w = (size_t)polys * (chain_idx + 1) * hp_.n;
    WITH_ARENA({
        u64 *a = ws(w), *b = ws(w);
        H2D(a, acc, w);
        H2D(b, x, w);
        launch_add(dlevel(chain_idx), a, b, polys, hp_.n, 1, st_);
        D2H(acc, a, w);
        tier1_done();
    });
}

void Engine::add_plain(u64 *ct, const u64 *pt, size_t pt_coeffs, int chain_idx)
{
    Enter g(this);
    TIER1_SLOTS();
    check_level(chain_idx);
    check_tier1_residues(ct, 1, chain_idx, "add_plain: operand holds a coefficient outside [0, q)");
    const size_t n = hp_.n, L = chain_idx + 1;
    if (pt_coeffs > n) throw std::invalid_argument("plaintext has too many coefficients");
    WITH_ARENA({
        u64 *c0 = ws(L * n), *p = ws(n);
        H2D(c0, ct, L * n);
        HIP_CHECK(hipMemsetAsync(p, 0, n * sizeof(u64), st_));
        H2D(p, pt, pt_coeffs);
        std::vector<PlainJob> jobs{ PlainJob{ c0, p } };
        { PROF(P_OTHER, 0); launch_add_plain(dlevel(chain_idx), upload_jobs(jobs), n, 1, st_); }
        D2H(ct, c0, L * n);
        tier1_done();
    });
}

void Engine::multiply(const u64 *a, const u64 *b, u64 *out3, int chain_idx)
{
    Enter g(this);
    TIER1_SLOTS();
    check_level(chain_idx);
    check_tier1_residues(a, 2, chain_idx, "multiply: operand holds a coefficient outside [0, q)");
    if (b != a) check_tier1_residues(b, 2, chain_idx, "multiply: operand holds a coefficient outside [0, q)");
    const size_t n = hp_.n, L = chain_idx + 1;
    const int E = hlevel(chain_idx).L + hlevel(chain_idx).nB + 1;
    const bool square = (a == b);
    WITH_ARENA({
        const int nop = square ? 1 : 2;
        u64 *in = ws((size_t)nop * 2 * L * n);
        H2D(in, a, 2 * L * n);
        if (!square) H2D(in + 2 * L * n, b, 2 * L * n);
        u64 *ext = ws((size_t)nop * 2 * E * n);
        { PROF(P_BEHZ_EXT, 0); launch_behz_ext(dlevel(chain_idx), hlevel(chain_idx).L, hlevel(chain_idx).nB, in, L * n, 1, ext, n, nop * 2, st_); }
        d_ntt(ext, (size_t)nop * 2 * E, map_ext(chain_idx), E, false, ext_primes_narrow_);
        u64 *d = ws((size_t)3 * E * n), *o = ws(3 * L * n);
        std::vector<TensorJob> tj{ TensorJob{ ext, square ? ext : ext + (size_t)2 * E * n, d } };
        { PROF(P_TENSOR, 0); launch_tensor(dlevel(chain_idx), upload_jobs(tj), n, 1, st_); }
        d_ntt(d, (size_t)3 * E, map_ext_fin(chain_idx), E, true, ext_primes_narrow_);        // the finish below applies the twist where it can
        std::vector<FinishJob> fj{ FinishJob{ d, o, 1, 0 } };
        { PROF(P_BEHZ_FINISH, 0); launch_behz_finish(dlevel(chain_idx), hlevel(chain_idx).L, hlevel(chain_idx).nB, upload_jobs(fj), false, n, 1, st_); }
        D2H(out3, o, 3 * L * n);
        tier1_done();
    });
}

void Engine::relinearize(u64 *ct3, const RelinKeys &rk, int chain_idx)
{
    Enter g(this);
    TIER1_SLOTS();
    check_level(chain_idx);
    check_tier1_residues(ct3, 3, chain_idx, "relinearize: operand holds a coefficient outside [0, q)");
    if (!hp_.using_keyswitching) throw std::logic_error("parameters do not support key switching");
    const size_t n = hp_.n, L = chain_idx + 1;
    WITH_ARENA({
        u64 *d = ws(3 * L * n);
        H2D(d, ct3, 3 * L * n);
        d_relinearize(d, 3 * L * n, 1, rk, chain_idx);
        D2H(ct3, d, 2 * L * n);
        tier1_done();
    });
}

void Engine::mod_switch_to_next(u64 *ct, int polys, int chain_idx)
{
    Enter g(this);
    TIER1_SLOTS();
    check_level(chain_idx);
    check_tier1_residues(ct, polys, chain_idx, "mod_switch_to_next: operand holds a coefficient outside [0, q)");
    if (chain_idx == 0) throw std::invalid_argument("end of modulus switching chain reached");
    const size_t n = hp_.n, L = chain_idx + 1;
    WITH_ARENA({
        u64 *d = ws(polys * L * n), *o = ws(polys * (L - 1) * n);
        H2D(d, ct, polys * L * n);
        { PROF(P_MODSWITCH, 0); launch_modswitch(dlevel(chain_idx), d, polys * L * n, polys, o, n, 1, st_); }
        D2H(ct, o, polys * (L - 1) * n);
        tier1_done();
    });
}

void Engine::clear_irrelevant_bits(u64 *ct, int polys)
{
    Enter g(this);
    TIER1_SLOTS();
    const size_t w = (size_t)polys * hp_.n;
    WITH_ARENA({
        u64 *d = ws(w);
        H2D(d, ct, w);
        launch_clear_bits(d, w, hp_.irrelevant_bit_count, st_);
        D2H(ct, d, w);
        tier1_done();
    });
}

// ============================================================================ tier 2: uploads
std::unique_ptr<RelinKeys> Engine::upload_relin_keys(const u64 *rk_host)
{
    Enter g(this);
    if (!hp_.using_keyswitching) throw std::logic_error("parameters do not support key switching");
    auto rk = std::make_unique<RelinKeys>();
    const size_t w = (size_t)(hp_.K - 1) * 2 * hp_.K * hp_.n;
    rk->data.alloc(w * sizeof(u64));
    HIP_CHECK(hipMemcpy(rk->data.p(), rk_host, w * sizeof(u64), hipMemcpyHostToDevice));
    return rk;
}

// ============================================================================ tier 2: ComputePowers
void Engine::build_schedule_for(Sched &s, const std::vector<char> &member)
{
    s = Sched{};
    const auto &nodes = dag_.nodes();
    const uint32_t max_power = *dag_.target_powers().rbegin();
    std::vector<char> is_parent(max_power + 1, 0);
    uint32_t depth = 0;
    for (auto &kv : nodes) {
        if (!member[kv.first]) continue;
        depth = std::max(depth, kv.second.depth);
        if (!kv.second.is_source()) { is_parent[kv.second.parents.first] = 1; is_parent[kv.second.parents.second] = 1; }
    }
    std::vector<PowersDag::PowersNode> order;
    for (auto &kv : nodes) if (member[kv.first]) order.push_back(kv.second);
    std::stable_sort(order.begin(), order.end(), [&](const auto &a, const auto &b) {
        if (a.depth != b.depth) return a.depth < b.depth;
        if (is_parent[a.power] != is_parent[b.power]) return is_parent[a.power] > is_parent[b.power];
        return a.power < b.power;
    });
    s.slot_of.assign(max_power + 1, -1);
    for (size_t i = 0; i < order.size(); i++) { s.slot_power.push_back(order[i].power); s.slot_of[order[i].power] = (int)i; }
    s.levels.assign(depth + 1, Sched::Level{ 0, 0, 0 });
    for (uint32_t d = 0; d <= depth; d++) {
        int s0 = -1, s1 = -1, sp = -1;
        for (size_t i = 0; i < order.size(); i++) {
            if (order[i].depth != d) continue;
            if (s0 < 0) s0 = (int)i;
            s1 = (int)i + 1;
            if (is_parent[order[i].power]) sp = (int)i + 1;
        }
        if (s0 < 0) s0 = s1 = 0;                      // no node of this subset at this depth
        if (sp < 0) sp = s0;
        s.levels[d] = Sched::Level{ s0, s1, sp };
    }
    for (size_t i = 0; i < order.size(); i++)
        if (!order[i].is_source())
            s.nodes.push_back({ (int)i, s.slot_of[order[i].parents.first], s.slot_of[order[i].parents.second] });
    const uint32_t ps = psu_.query_params.ps_low_degree;
    for (uint32_t p : dag_.target_powers()) {
        if (!member[p]) continue;
        if (!ps || p <= ps) s.low_powers.push_back(p);
        else s.high_powers.push_back(p);
    }
}

void Engine::build_schedule()
{
    const auto &nodes = dag_.nodes();
    const uint32_t max_power = *dag_.target_powers().rbegin();
    build_schedule_for(sched_, std::vector<char>(max_power + 1, 1));
    // The powers that stay at the low level and the Paterson-Stockmeyer high powers usually descend from different
    // query powers (all four reference parameter sets).  Then ComputePowers is two independent chains: the second one
    // runs on its own stream, next to the first and to the BinBundle inner products that only need the low powers.
    split_ok_ = false;
    if (sched_.high_powers.empty() || sched_.low_powers.empty() || dag_.depth() == 0) return;
    auto closure = [&](const std::vector<uint32_t> &targets) {
        std::vector<char> m(max_power + 1, 0);
        std::vector<uint32_t> stack(targets.begin(), targets.end());
        while (!stack.empty()) {
            const uint32_t p = stack.back();
            stack.pop_back();
            if (m[p]) continue;
            m[p] = 1;
            const auto &nd = nodes.at(p);
            if (!nd.is_source()) { stack.push_back(nd.parents.first); stack.push_back(nd.parents.second); }
        }
        return m;
    };
    const auto ml = closure(sched_.low_powers), mh = closure(sched_.high_powers);
    for (uint32_t p = 0; p <= max_power; p++) if (ml[p] && mh[p]) return;
    build_schedule_for(sched_low_, ml);
    build_schedule_for(sched_high_, mh);
    split_ok_ = true;
}

// One walk over a (sub)schedule of the PowersDag on the current lane: sources (dag_sources), the level-synchronous products
// (dag_level(d), d = 1 ..), and the final per-power conversions (dag_outputs) (receiver_osn.cpp:395-488).
// The steps of one walk must run in order on one lane; DagRun carries the walk's buffers between them, so two walks
// (the halves of a split DAG) can be interleaved level by level on two lanes.
struct Engine::DagRun {
    const Sched &s; int nb; size_t n, Lf, Ef, slot_w;       // slot_w: (c0, c1, c2 scratch) per power and bundle index
    u64 *pwf = nullptr, *ext = nullptr, *dbuf = nullptr; size_t arena_mark = 0; int ext_done = -1;   // ext_done: level whose parents are already extended
    DagRun(const Engine &e, const Sched &s_, int nb_)
        : s(s_), nb(nb_), n(e.hp_.n), Lf(e.hp_.first_chain_idx + 1),
          Ef(e.dlevel(e.hp_.first_chain_idx) ? (size_t)(e.hlevel(e.hp_.first_chain_idx).L + e.hlevel(e.hp_.first_chain_idx).nB + 1) : 0), slot_w(3 * Lf * n) {}
    u64 *slot_ptr(int slot, int b) const { return pwf + ((size_t)slot * nb + b) * slot_w; }
    u64 *ext_ptr(int slot, int b) const { return ext + ((size_t)slot * nb + b) * 2 * Ef * n; }
};

// workspace + sources (receiver_osn.cpp:304-317)
void Engine::dag_sources(DagRun &run, const u64 *const *src, bool on_device)
{
    const Sched &s = run.s;
    const size_t n = run.n, Lf = run.Lf, P = s.slot_power.size();
    const int first = hp_.first_chain_idx, nb = run.nb;
    run.pwf = ws(P * nb * run.slot_w);
    int si = 0;
    std::vector<CtJob> cj;                               // device-resident sources: one gather launch
    for (auto &kv : dag_.nodes()) {
        if (!kv.second.is_source()) continue;
        if (s.slot_of[kv.first] < 0) { si++; continue; }        // belongs to the other half of a split DAG
        for (int b = 0; b < nb; b++) {
            const u64 *sp = src[(size_t)b * dag_.source_count() + si];
            u64 *slot = run.slot_ptr(s.slot_of[kv.first], b);
            if (on_device) cj.push_back(CtJob{ sp, slot });
            else {                                       // host sources: a plain copy, then the same check in place (round 6)
                H2D(slot, sp, 2 * Lf * n);
                cj.push_back(CtJob{ slot, slot });
            }
        }
        si++;
    }
    if (!cj.empty()) { PROF(P_OTHER, 0); launch_copy_sources(upload_jobs(cj), 2 * Lf * n, (int)cj.size(), dlevel(first), (int)Lf, n, bad_source_ + query_seq_ % BAD_SLOTS, query_seq_, st_); }
    if (s.levels.size() > 1) {
        run.ext = ws(P * nb * 2 * run.Ef * n);
        size_t max_nodes = 0;
        for (size_t d = 1; d < s.levels.size(); d++) max_nodes = std::max(max_nodes, (size_t)(s.levels[d].s1 - s.levels[d].s0));
        run.dbuf = ws(max_nodes * nb * 3 * run.Ef * n);
    }
    run.arena_mark = arena_off_;
}

// the products of depth d >= 1 (nothing when the schedule is shallower)
void Engine::dag_level(DagRun &run, size_t d, const RelinKeys *rk)
{
    const Sched &s = run.s;
    if (d >= s.levels.size()) return;
    const size_t n = run.n, Lf = run.Lf, Ef = run.Ef;
    const int first = hp_.first_chain_idx, nb = run.nb;
    arena_off_ = run.arena_mark;
    // extend + NTT the parents that became available at depth d-1
    const auto &pl = s.levels[d - 1];
    const int npar = pl.sp - pl.s0;
    if (npar > 0) {
        // (parents that came out of a key switch were extended by its mod-down kernel: run.ext_done)
        if (run.ext_done != (int)d - 1) { PROFW(P_BEHZ_EXT, (size_t)npar * nb * 2 * n * (Lf + Ef)); launch_behz_ext(dlevel(first), hlevel(first).L, hlevel(first).nB, run.slot_ptr(pl.s0, 0), run.slot_w, 2, run.ext_ptr(pl.s0, 0), n, npar * nb, st_); }
        d_ntt(run.ext_ptr(pl.s0, 0), (size_t)npar * nb * 2 * Ef, map_ext(first), (int)Ef, false, ext_primes_narrow_);
    }
    const auto &cl = s.levels[d];
    const int nn = cl.s1 - cl.s0;
    if (nn <= 0) return;
    std::vector<TensorJob> tj;
    std::vector<FinishJob> fj;
    for (auto &nd : s.nodes) {
        if (nd[0] < cl.s0 || nd[0] >= cl.s1) continue;
        for (int b = 0; b < nb; b++) {
            u64 *dd = run.dbuf + ((size_t)(nd[0] - cl.s0) * nb + b) * 3 * Ef * n;
            tj.push_back(TensorJob{ run.ext_ptr(nd[1], b), run.ext_ptr(nd[2], b), dd });
            fj.push_back(FinishJob{ dd, run.slot_ptr(nd[0], b), 1, 0 });
        }
    }
    if (fuse_tensor_) {                                                                                              // :422/:424
        PROF(P_NTT_FUSED, tj.size() * 3 * Ef);
        launch_intt_tensor(hp_.logn, upload_jobs(tj), (int)tj.size(), (int)Ef, Ef * n, nullptr, 0, tabs(), map_ext_fin(first), (int)Ef, st_, sw_.ntt_latency_limbs);
    } else {
        { PROF(P_TENSOR, 0); launch_tensor(dlevel(first), upload_jobs(tj), n, (int)tj.size(), st_); }
        d_ntt(run.dbuf, (size_t)nn * nb * 3 * Ef, map_ext_fin(first), (int)Ef, true, ext_primes_narrow_);
    }
    { PROFW(P_BEHZ_FINISH, fj.size() * 3 * n * (Ef + Lf)); launch_behz_finish(dlevel(first), hlevel(first).L, hlevel(first).nB, upload_jobs(fj), false, n, (int)fj.size(), st_); }
    if (hp_.using_keyswitching) {                                                                                    // :431
        const int npar_here = (d + 1 < s.levels.size()) ? (cl.sp - cl.s0) : 0;
        if (d_relinearize(run.slot_ptr(cl.s0, 0), run.slot_w, nn * nb, *rk, first, npar_here ? run.ext_ptr(cl.s0, 0) : nullptr, npar_here * nb))
            run.ext_done = (int)d;
    }
}

// final per-power conversions (receiver_osn.cpp:459-487)
void Engine::dag_outputs(DagRun &run, Powers &pw, bool do_low, bool do_high)
{
    const Sched &s = run.s;
    const size_t n = run.n, Lf = run.Lf;
    const int first = hp_.first_chain_idx, high = hp_.clamp_chain_idx(1), nb = run.nb;
    const size_t Lh = high + 1, Eh = hlevel(high).L + hlevel(high).nB + 1;
    arena_off_ = run.arena_mark;
    auto convert = [&](const std::vector<uint32_t> &powers, int target, u64 *out) {
        if (powers.empty()) return;
        const int cnt = (int)powers.size() * nb;
        std::vector<CtJob> jobs;
        int lvl = first;
        u64 *cur = nullptr;
        auto dst_for = [&](int level_after) -> u64 * {
            return level_after == target ? out : ws((size_t)cnt * 2 * (level_after + 1) * n);
        };
        if (first == target) {
            for (size_t i = 0; i < powers.size(); i++)
                for (int b = 0; b < nb; b++)
                    jobs.push_back(CtJob{ run.slot_ptr(s.slot_of[powers[i]], b), out + ((size_t)b * powers.size() + i) * 2 * Lf * n });
            { PROF(P_OTHER, 0); launch_copy_jobs(upload_jobs(jobs), 2 * Lf * n, cnt, st_); }
            return;
        }
        cur = dst_for(first - 1);
        for (size_t i = 0; i < powers.size(); i++)
            for (int b = 0; b < nb; b++)
                jobs.push_back(CtJob{ run.slot_ptr(s.slot_of[powers[i]], b), cur + ((size_t)b * powers.size() + i) * 2 * (Lf - 1) * n });
        { PROFW(P_MODSWITCH, (size_t)cnt * 2 * n * (2 * Lf - 1)); launch_modswitch_jobs(dlevel(first), upload_jobs(jobs), 2, n, cnt, st_); }                     // :463,471,478
        lvl = first - 1;
        while (lvl > target) {
            u64 *nxt = dst_for(lvl - 1);
            { PROFW(P_MODSWITCH, (size_t)cnt * 2 * n * (2 * lvl + 1)); launch_modswitch(dlevel(lvl), cur, (size_t)2 * (lvl + 1) * n, 2, nxt, n, cnt, st_); }
            cur = nxt;
            lvl--;
        }
    };
    if (do_low && first == pw.low_level && !s.low_powers.empty()) {
        // no level change: the forward NTT (:467,475) reads the slots and writes the packed output directly
        const size_t np = s.low_powers.size();
        std::vector<const u64 *> srcp(np * nb * 2 * Lf);
        for (int b = 0; b < nb; b++)
            for (size_t i = 0; i < np; i++)
                for (size_t pl = 0; pl < 2 * Lf; pl++)
                    srcp[(((size_t)b * np + i) * 2 * Lf) + pl] = run.slot_ptr(s.slot_of[s.low_powers[i]], b) + pl * n;
        // (limb j of a slot is already a canonical residue of q_j: nothing to reduce)
        bool nored = hp_.logn <= 14;
        for (size_t j = 0; j < Lf && nored; j++) nored = ntt_gather_nored_ok(hp_.key_q[j], hp_.key_q[j], hp_.logn);
        PROF(P_NTT_FWD, srcp.size());
        launch_ntt_gather(hp_.logn, upload_jobs(srcp), pw.low.u(), srcp.size(), tabs(), map_ct(), (int)Lf, st_, nored, sw_.ntt_latency_limbs, data_primes_narrow_);
    } else if (do_low) {
        convert(s.low_powers, pw.low_level, pw.low.u());
        d_ntt_ct(pw.low.u(), (size_t)pw.n_low * nb * 2, pw.low_level, false);                         // :467,475
    }
    if (do_high && pw.n_high) {
        convert(s.high_powers, high, pw.high.u());
        // derived form used by eval_patstock's ct x ct products and coefficient-form plaintext products
        { PROFW(P_BEHZ_EXT, (size_t)pw.n_high * nb * 2 * n * (Lh + Eh)); launch_behz_ext(dlevel(high), hlevel(high).L, hlevel(high).nB, pw.high.u(), Lh * n, 1, pw.hext.u(), n, (int)(pw.n_high * nb * 2), st_); }
        d_ntt(pw.hext.u(), (size_t)pw.n_high * nb * 2 * Eh, map_ext(high), (int)Eh, false, ext_primes_narrow_);
    }
}

// the whole of one walk on the current lane
void Engine::dag_walk(const Sched &s, int nb, const u64 *const *src, bool on_device, const RelinKeys *rk, Powers &pw)
{
    DagRun r(*this, s, nb);
    dag_sources(r, src, on_device);
    for (size_t d = 1; d < s.levels.size(); d++) dag_level(r, d, rk);
    dag_outputs(r, pw, true, true);
}

std::unique_ptr<Powers> Engine::compute_powers(const uint32_t *bundle_indices, int nb, const u64 *const *src, bool on_device,
                                               const RelinKeys *rk)
{
    Enter g(this);
    if (!has_psu_) throw std::logic_error("context was created without PSUParams");
    if (nb <= 0) throw std::invalid_argument("no bundle indices given");
    if (hp_.using_keyswitching && dag_.depth() > 0 && !rk) throw std::invalid_argument("relinearization keys are required");
    // one coefficient prime = no key switching: the reference then leaves every product unrelinearised (receiver_osn.cpp:427-432)
    // and multiplies the longer ciphertexts further: a path of its own (every shipped single-prime set has depth 0)
    if (nks_) return compute_powers_nks(bundle_indices, nb, src, on_device);
    const Sched &s = sched_;
    const size_t n = hp_.n;
    job_seq_base_ = 0;                                       // job-cache slots 0..255: ComputePowers
    const int high = hp_.clamp_chain_idx(1), low = hp_.clamp_chain_idx(2);
    const uint32_t ps = psu_.query_params.ps_low_degree;
    const int low_target = ps ? low : high;                 // receiver_osn.cpp:459-487
    const size_t Ll_ = low_target + 1, Lh_ = high + 1, Eh_ = hlevel(high).L + hlevel(high).nB + 1;
    const size_t need_low = s.low_powers.size() * nb * 2 * Ll_ * n * sizeof(u64);
    const size_t need_high = s.high_powers.size() * nb * 2 * Lh_ * n * sizeof(u64);
    const size_t need_hext = s.high_powers.size() * nb * 2 * Eh_ * n * sizeof(u64);
    std::unique_ptr<Powers> pw;
    // (round 4) a pooled buffer whose last reader -- the evaluation of the query in front -- is still running would make this
    // query's second stream wait for that evaluation's end; with the caller's overlap promise the engine rather keeps TWO buffers of a shape and
    // takes the one whose reader is done (a caller that frees its powers right after queueing the evaluation, as the reference's
    // RunQuery does, then gets the alternation for free: 68 MB more at 16M-4096)
    {
        // (the rule itself: sched_policy.h, pick_pooled_buffer -- enumerated on the CPU tier)
        std::vector<PoolEntryState> st(powers_pool_.size());
        for (size_t i = 0; i < powers_pool_.size(); i++) {
            Powers &c = *powers_pool_[i];
            st[i].fits = c.low.bytes() == need_low && c.high.bytes() == need_high && c.hext.bytes() == need_hext;
            st[i].last_use_set = c.last_use_set;
            st[i].last_use_done = st[i].fits && inputs_ready_ && c.last_use_set && hipEventQuery(c.last_use) == hipSuccess;
        }
        const int pick = pick_pooled_buffer(st.data(), st.size(), inputs_ready_);
        if (pick >= 0) {
            pw = std::move(powers_pool_[pick]);
            powers_pool_.erase(powers_pool_.begin() + pick);
        }
    }
    const bool recycled = (bool)pw;
    // The ordering rules -- which walk, behind which events -- are a pure function of this state (sched_policy.h, plan_walk; every
    // state is enumerated against the no-unordered-writer invariant in tests/test_host_logic.py).
    WalkState wst{};
    wst.recycled = recycled;
    wst.last_use_set = recycled && pw->last_use_set;
    wst.last_use_done = wst.last_use_set && hipEventQuery(pw->last_use) == hipSuccess;
    wst.high_async = recycled && pw->high_async && pw->high_ready;
    wst.split_ok = split_ok_;
    wst.prof_on = prof_on_;
    wst.split_mode = two_stream_mode_ >= 0 ? two_stream_mode_ : sw_.two_stream_default;       // API override, then environment
    wst.pipe_cp = pipe_cp_;
    wst.force_pipe = force_pipe_;
    wst.inputs_ready = inputs_ready_;
    wst.on_device = on_device;
    // "busy": an evaluation queued earlier is still running (a query that finds the device idle takes the split walk: the merged
    // chain is ~3 % slower for one query alone, profiles/r02_pipe_sweep.txt; a stream of queued queries takes the pipelined one)
    if (pipe_cp_ && inflight_count_ > 0 && !inflight_.empty())
        wst.device_busy = hipEventQuery(inflight_[(inflight_head_ + inflight_count_ - 1) % inflight_.size()]) == hipErrorNotReady;
    const WalkPlan plan = plan_walk(wst);
    // a pooled buffer whose high half was produced on the second stream and never consumed: the main stream must not
    // overwrite it before those kernels have finished
    if (plan.main_waits_high_ready) HIP_CHECK(hipStreamWaitEvent(st_, pw->high_ready, 0));
    if (!pw) pw = std::make_unique<Powers>();
    if (++query_seq_ == 0) query_seq_ = 1;                   // (0 = "never computed")
    pw->seq = query_seq_;
    pw->nb = nb;
    pw->bundle_indices.assign(bundle_indices, bundle_indices + nb);
    pw->low_level = low_target;
    pw->high_level = high;
    pw->n_low = (uint32_t)s.low_powers.size();
    pw->n_high = (uint32_t)s.high_powers.size();
    if (!recycled) {
        counters_[C_POWERS_ALLOC]++;
        pw->low.alloc(need_low);
        if (pw->n_high) {
            pw->high.alloc(need_high);
            pw->hext.alloc(need_hext);
        }
    }

    struct LaneGuard { Engine *e; ~LaneGuard() { e->switch_lane(0); } } lane_guard{ this };
    PhaseSpan cp_span;
    if (phase_on_) {
        phase_close_query();
        cp_span.phase = PH_COMPUTE_POWERS;
        cp_span.a = phase_event(st_);
        query_start_ = phase_event(st_);
    }
    // Two-stream walk: the high-power half of the DAG runs on the second stream next to the low-power half and to the
    // BinBundle inner products.  Measured on 16M-4096 (tools/pipe_sweep.py, tools/rank_cost.py): 3.84 ->
    // 3.65 ms for the whole query (four bundle indices), 0.95 -> 0.86 ms per rank with one bundle index.  Default: on
    // whenever the PowersDag splits; APSU_HE_SPLIT=0/1 (read at apsu_he_create) or apsu_he_set_two_stream force it.  Event profiling always takes
    // the one-stream walk: a launch bracketed by events next to another stream's kernels measures the sharing, not the kernel.
    const bool split = plan.walk != WALK_ONE_STREAM;         // (host inputs are uploaded per lane and end with a sync)
    pw->high_async = split;
    if (split && !pw->high_ready) HIP_CHECK(hipEventCreateWithFlags(&pw->high_ready, hipEventDisableTiming));
    // Pipelined queries (round 4): the WHOLE walk on the second stream -- one merged chain of launches -- next to the evaluation of
    // the query in front, the main stream only evaluates: -2.5 % on the rate of queued 16M-4096 queries, -7.7 % on the N = 8 shard
    // (profiles/r04_ab_pipe_cp.txt).  Needs the caller's apsu_he_set_query_overlap promise; only while an evaluation queued earlier is
    // still running and only into a buffer nobody reads any more (plan_walk).  `last_use` is consumed here and set again by
    // eval_bundles alone: a buffer that was computed and given back without an evaluation keeps no mark and takes the conservative order.
    const bool pipe = plan.walk == WALK_PIPELINED;
    pw->low_async = pipe;
    WITH_ARENA({
        for (hipEvent_t *e : { &cp_span.b, &cp_span.b2 }) if (*e) { phase_pool_.push_back(*e); *e = nullptr; }   // a retry after arena growth
        if (pipe) {
            switch_lane(1);
            if (plan.side_waits_last_use) HIP_CHECK(hipStreamWaitEvent(st_, pw->last_use, 0));
            dag_walk(sched_, nb, src, on_device, rk, *pw);
            HIP_CHECK(hipEventRecord(pw->high_ready, st_));
            switch_lane(0);
        } else if (!split) {
            dag_walk(sched_, nb, src, on_device, rk, *pw);
        } else {
            // everything queued so far on the main stream (the previous query's evaluation may still read a pooled
            // Powers buffer) precedes the second stream's work; the two walks are queued level by level so that
            // both streams have work from the start
            DagRun rl(*this, sched_low_, nb), rh(*this, sched_high_, nb);
            const size_t depth = std::max(sched_low_.levels.size(), sched_high_.levels.size());
            // (round 4: with device-resident inputs that the caller has declared complete -- apsu_he_set_query_overlap; lane 1 reads
            //  the sources and the relinearisation keys, which a caller may otherwise still be producing on the main stream -- the
            //  second stream waits for the LAST READER of this powers buffer -- the
            //  evaluation that used it before it went back to the pool -- not for everything the main stream has queued: the next
            //  query's high-power chain then runs next to the tail of the query in front of it, whose launches leave CUs idle)
            //  (plan.side_waits_main / side_waits_last_use; a pooled buffer whose reader left no mark waits for all)
            if (plan.side_waits_main) HIP_CHECK(hipEventRecord(ev_main_, st_));
            dag_sources(rl, src, on_device);
            switch_lane(1);
            if (plan.side_waits_main) HIP_CHECK(hipStreamWaitEvent(st_, ev_main_, 0));
            else if (plan.side_waits_last_use) HIP_CHECK(hipStreamWaitEvent(st_, pw->last_use, 0));
            dag_sources(rh, src, on_device);
            for (size_t d = 1; d < depth; d++) {
                switch_lane(0);
                dag_level(rl, d, rk);
                switch_lane(1);
                dag_level(rh, d, rk);
            }
            switch_lane(0);
            dag_outputs(rl, *pw, true, false);
            switch_lane(1);
            dag_outputs(rh, *pw, false, true);
            // (starting the high-power chain only when the low-power chain -- the evaluation's critical path -- has finished was
            //  measured in round 3: level on the whole query, 21 % slower on the N = 8 shard; profiles/r03_ab_fusions.txt)
            HIP_CHECK(hipEventRecord(pw->high_ready, st_));
            if (phase_on_ && cp_span.a && !cp_span.b2) cp_span.b2 = phase_event(st_);
            switch_lane(0);
        }
        if (phase_on_ && cp_span.a && !cp_span.b) cp_span.b = phase_event(st_);
        // device-resident inputs: no sync, consumers (eval_bundles, powers_download) are ordered on / synchronise
        // with the engine's streams.  Host inputs: the caller's buffers must have been consumed before returning.
        if (!on_device) sync();
    });
    if (phase_on_ && cp_span.a && cp_span.b) phase_spans_.push_back(cp_span);
    if (pipe) counters_[C_PIPELINED]++;                      // (once per call: the walk above is queued again after an arena growth)
    pw->last_use_set = false;                               // consumed above; only an evaluation of THESE powers sets it again
    return pw;
}

void Engine::download_power(const Powers &pw, uint32_t bundle_idx, uint32_t power, u64 *out, size_t capacity_words, int *chain_idx,
                            int *is_ntt)
{
    Enter g(this);
    if (!has_psu_) throw std::invalid_argument("context has no PSUParams");
    const int b = pw.slot_of(bundle_idx);
    if (b < 0) throw std::invalid_argument("bundle index not present");
    const uint32_t ps = psu_.query_params.ps_low_degree;
    const bool low = !ps || power <= ps;
    const int lvl = low ? pw.low_level : pw.high_level;
    uint32_t idx;
    if (low) {
        if (power < 1 || power > pw.n_low) throw std::invalid_argument("power not available");
        idx = power - 1;
    } else {
        if (power % (ps + 1) != 0 || power / (ps + 1) > pw.n_high) throw std::invalid_argument("power not available");
        idx = power / (ps + 1) - 1;
    }
    const size_t words = (size_t)power_size(power) * (lvl + 1) * hp_.n;               // the stored slot may be zero-padded beyond that
    if (capacity_words < words) throw std::invalid_argument("output buffer too small");
    sync();
    check_sources(pw);
    const u64 *src = (low ? pw.low.u() : pw.high.u()) + ((size_t)b * (low ? pw.n_low : pw.n_high) + idx) * pw.polys * (lvl + 1) * hp_.n;
    HIP_CHECK(hipMemcpy(out, src, words * sizeof(u64), hipMemcpyDeviceToHost));
    if (chain_idx) *chain_idx = lvl;
    if (is_ntt) *is_ntt = low ? 1 : 0;
}

// ============================================================================ N3: seeded objects expanded on the device
void Engine::seed_expand(int chain_idx, int count, const u64 *seeds, u64 *const *dst)
{
    Enter g(this);
    if (count <= 0) return;
    if (!seeds || !dst) throw std::invalid_argument("null argument");
    const bool key_level = chain_idx < 0 || chain_idx == hp_.K - 1;
    if (!key_level) check_level(chain_idx);
    for (int i = 0; i < count; i++) if (!dst[i]) throw std::invalid_argument("null destination");
    const int L = key_level ? hp_.K : chain_idx + 1;
    TIER1_SLOTS();
    job_seq_ = job_seq_base_;
    // The device list holds 8192 rejected words per object.  The rejection rate is ~q / 2^64 per word, so ~60-bit primes with a large
    // L * n may legitimately exceed it (and L may exceed the device tables): those objects are expanded by the host's
    // sample_poly_uniform (seal_codec.cpp) and uploaded -- slower, same words.  APSU_HE_SEED_EXPAND_HOST=1 forces that path (tests).
    bool on_device = queue_seed_expand(L, count, seeds, dst);
    if (on_device) {
        sync();
        on_device = !seeds_overflowed(count);                    // more rejected words than the device list holds: the host redoes these objects
    }
    if (!on_device) host_seed_expand(L, count, seeds, dst);
}

// ============================================================================ N4: masks, packing, loopback decrypt
static uint32_t plain_modulus_len(u64 t)
{
    // receiver_osn.cpp:54-57: smallest len with (1 << len) - 1 >= plain_modulus
    uint32_t len = 1;
    while ((((u64)1 << len) - 1) < t) len++;
    return len;
}

void Engine::mask_generate(u64 seed, uint32_t count, u64 *masks_dev, u64 *values_host, u64 *blocks_host)
{
    mask_generate_impl(count, masks_dev, values_host, blocks_host, [&](u64 *vals, size_t words) { launch_fill_random(vals, words, seed, hp_.t, st_); });
}

void Engine::mask_generate_blake2xb(const u64 seed[8], u64 first_value, uint32_t count, u64 *masks_dev, u64 *values_host, u64 *blocks_host)
{
    Blake2xbSeed sd;
    for (int i = 0; i < 8; i++) sd.w[i] = seed[i];
    mask_generate_impl(count, masks_dev, values_host, blocks_host,
                       [&](u64 *vals, size_t words) { launch_fill_blake2xb(vals, words, sd, first_value, hp_.t, st_); });
}

void Engine::mask_generate_impl(uint32_t count, u64 *masks_dev, u64 *values_host, u64 *blocks_host, const std::function<void(u64 *, size_t)> &fill)
{
    Enter g(this);
    if (!has_psu_) throw std::logic_error("context was created without PSUParams");
    if (!hp_.batching) throw std::logic_error("plain_modulus does not support batching");
    if (!count) return;
    const size_t n = hp_.n;
    const uint32_t items = psu_.items_per_bundle, felts = psu_.item_params.felts_per_item;
    const int tid = hp_.plain_id();
    TIER1_SLOTS();
    WITH_ARENA({
        u64 *vals = ws((size_t)count * n);
        { PROF(P_OTHER, 0); fill(vals, (size_t)count * n); }                                                       // :248-251
        // BatchEncoder::encode (:271): slot permutation, inverse negacyclic NTT mod t
        { PROF(P_OTHER, 0); launch_scatter_slots(vals, reinterpret_cast<const uint32_t *>(d_slot_map_.p()), masks_dev, n, (int)count, st_); }
        d_ntt(masks_dev, count, map_ct() + tid, 1, true, false);
        if (blocks_host) {                                                                                        // :256-266
            u64 *blk = ws((size_t)count * items * 2);
            { PROF(P_OTHER, 0); launch_pack_blocks(vals, n, items, felts, plain_modulus_len(hp_.t), blk, (int)count, st_); }
            D2H(blocks_host, blk, (size_t)count * items * 2);
        }
        if (values_host) D2H(values_host, vals, (size_t)count * n);
        sync();
    });
}

void Engine::decrypt_decode(const u64 *sk_ntt_host, const u64 *cts, bool on_device, uint32_t count, u64 *values_host, u64 *blocks_host, int *budget_bits,
                            bool sk_on_device, u64 *values_dev)
{
    Enter g(this);
    if (!has_psu_) throw std::logic_error("context was created without PSUParams");
    if (!hp_.batching) throw std::logic_error("plain_modulus does not support batching");
    if (!count) return;
    const size_t n = hp_.n;
    const uint32_t items = psu_.items_per_bundle, felts = psu_.item_params.felts_per_item;
    const int tid = hp_.plain_id();
    for (size_t k = 0; !sk_on_device && k < n; k++)
        if (sk_ntt_host[k] >= hp_.key_q[0]) throw std::invalid_argument("secret key is not reduced modulo q_0");
    TIER1_SLOTS();
    WITH_ARENA({
        const u64 *sk = sk_ntt_host;                             // (sk_on_device: the engine's own key, used where it lies)
        if (!sk_on_device) {
            u64 *staged = ws(n);
            H2D(staged, sk_ntt_host, n);
            sk = staged;
        }
        const u64 *ct = cts;
        if (!on_device) {
            u64 *c = ws((size_t)count * 2 * n);
            H2D(c, cts, (size_t)count * 2 * n);
            ct = c;
        }
        // c1 -> NTT, (.) s, INTT  (dot_product_ct_sk_array at one limb)
        u64 *v = ws((size_t)count * n);
        std::vector<CtJob> cj;
        for (uint32_t i = 0; i < count; i++) cj.push_back(CtJob{ ct + ((size_t)i * 2 + 1) * n, v + (size_t)i * n });
        { PROF(P_OTHER, 0); launch_copy_jobs(upload_jobs(cj), n, (int)count, st_); }
        d_ntt(v, count, map_ct(), 1, false, data_primes_narrow_);
        { PROF(P_OTHER, 0); launch_dyadic_plain(dlevel(0), v, sk, v, 1, n, (int)count, 0, st_); }
        d_ntt(v, count, map_ct(), 1, true, data_primes_narrow_);
        // x = c0 + v; m = round(t x / q_0) mod t
        u64 *pt = ws((size_t)count * n);
        std::vector<u64> worst_host;
        if (budget_bits) {
            u64 *worst = ws(count);
            worst_host.resize(count);
            HIP_CHECK(hipMemsetAsync(worst, 0, count * sizeof(u64), st_));
            { PROF(P_OTHER, 0); launch_decrypt_round_budget(ct, 2 * n, v, hp_.key_q[0], hp_.t, pt, n, (int)count, worst, st_); }
            D2H(worst_host.data(), worst, count);
        } else
        { PROF(P_OTHER, 0); launch_decrypt_round(ct, 2 * n, v, hp_.key_q[0], hp_.t, pt, n, (int)count, st_); }
        // BatchEncoder::decode: forward NTT mod t, slot gather
        d_ntt(pt, count, map_ct() + tid, 1, false, false);
        u64 *vals = ws((size_t)count * n);
        { PROF(P_OTHER, 0); launch_gather_slots(pt, reinterpret_cast<const uint32_t *>(d_slot_map_.p()), vals, n, (int)count, st_); }
        if (blocks_host) {                                                                      // sender_osn.cpp:684-690
            u64 *blk = ws((size_t)count * items * 2);
            { PROF(P_OTHER, 0); launch_pack_blocks(vals, n, items, felts, plain_modulus_len(hp_.t), blk, (int)count, st_); }
            D2H(blocks_host, blk, (size_t)count * items * 2);
        }
        if (values_host) D2H(values_host, vals, (size_t)count * n);
        if (values_dev) D2D(values_dev, vals, (size_t)count * n);
        sync();
        // Decryptor::invariant_noise_budget: floor(log2(q_0 / (2 |t x mod q_0|))), the whole of q_0 for a noiseless result
        for (uint32_t i = 0; budget_bits && i < count; i++) {
            const unsigned __int128 q0 = hp_.key_q[0], w = worst_host[i];
            int bits = 0;
            while (w && (w << (bits + 1)) < q0) bits++;
            budget_bits[i] = w ? bits : 64 - __builtin_clzll(hp_.key_q[0]);
        }
    });
}

// ============================================================================ N5: the querier's side (query_side.h)
void Engine::check_key_residues(const u64 *sk, int limbs) const
{
    for (int j = 0; j < limbs; j++)
        for (size_t k = 0; k < hp_.n; k++)
            if (sk[(size_t)j * hp_.n + k] >= hp_.key_q[j]) throw std::invalid_argument("secret key is not reduced modulo its limb's prime");
}

static Blake2xbSeed master_seed(const u64 seed[8])
{
    Blake2xbSeed sd;
    for (int i = 0; i < 8; i++) sd.w[i] = seed[i];
    return sd;
}

void Engine::host_seed_expand(int L, int count, const u64 *seeds, u64 *const *dst)
{
    std::vector<u64> q(hp_.key_q.begin(), hp_.key_q.begin() + L), buf((size_t)L * hp_.n);
    for (int i = 0; i < count; i++) {
        sealio::sample_poly_uniform(seeds + (size_t)i * 8, q.data(), (size_t)L, hp_.n, buf.data());
        HIP_CHECK(hipMemcpyAsync(dst[i], buf.data(), buf.size() * sizeof(u64), hipMemcpyHostToDevice, st_));
        sync();                                                  // buf is reused
    }
}

bool Engine::queue_seed_expand(int L, int count, const u64 *seeds, u64 *const *dst)
{
    if (L > DMAXL || sw_.seed_expand_host) return false;
    const bool key_view = L == hp_.K && !key_level_.empty();     // the key level is not a data level: its moduli-only view (engine.h)
    if (key_view && !d_key_level_.p()) {
        d_key_level_.alloc(sizeof(DevLevel));
        HIP_CHECK(hipMemcpy(d_key_level_.p(), key_level_.data(), sizeof(DevLevel), hipMemcpyHostToDevice));
    }
    const DevLevel *lv = key_view ? reinterpret_cast<const DevLevel *>(d_key_level_.p()) : dlevel(L - 1);
    const std::vector<u64> mm(max_multiple_.begin(), max_multiple_.begin() + L);
    std::vector<SeedJob> jobs(count);
    for (int i = 0; i < count; i++) {
        for (int k = 0; k < 8; k++) jobs[i].seed.w[k] = seeds[(size_t)i * 8 + k];
        jobs[i].dst = dst[i];
    }
    const size_t need = ((size_t)count * (1 + 8192) + 1) * sizeof(u32);
    if (d_seed_rej_.bytes() < need) {
        sync();
        d_seed_rej_.alloc(need * 2);
        HIP_CHECK(hipMemsetAsync(d_seed_rej_.p(), 0, d_seed_rej_.bytes(), st_));
    }
    u32 *rej = reinterpret_cast<u32 *>(d_seed_rej_.p());
    int *overflow = reinterpret_cast<int *>(rej + (size_t)count * (1 + 8192));
    HIP_CHECK(hipMemsetAsync(overflow, 0, sizeof(int), st_));
    { PROF(P_OTHER, 0); launch_seed_expand(upload_jobs(jobs), count, lv, L, upload_jobs(mm), hp_.n, rej, overflow, st_); }
    return true;
}

// after a sync: did some object reject more words than the device lists hold?  (then the lists are cleared for their next use)
bool Engine::seeds_overflowed(int count)
{
    int h = 0;
    HIP_CHECK(hipMemcpy(&h, reinterpret_cast<u32 *>(d_seed_rej_.p()) + (size_t)count * (1 + 8192), sizeof(int), hipMemcpyDeviceToHost));
    if (h) {
        HIP_CHECK(hipMemsetAsync(d_seed_rej_.p(), 0, d_seed_rej_.bytes(), st_));
        sync();
    }
    return h != 0;
}

void Engine::keygen(const u64 seed[8], u64 *sk_ntt_host, bool sk_on_device)
{
    Enter g(this);
    const size_t n = hp_.n;
    const int K = hp_.K;
    TIER1_SLOTS();
    WITH_ARENA({
        signed char *small = reinterpret_cast<signed char *>(ws(n / 8));
        u64 *sk = ws((size_t)K * n);
        { PROF(P_OTHER, 0); launch_sample_ternary(master_seed(seed), small, n, st_); }
        { PROF(P_OTHER, 0); launch_small_lift(dkey(), small, sk, K, n, 1, st_); }
        d_ntt(sk, K, map_ct(), K, false, data_primes_narrow_);
        HIP_CHECK(hipMemcpyAsync(sk_ntt_host, sk, (size_t)K * n * sizeof(u64), sk_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st_));
        sync();
    });
}

void Engine::relin_keygen(const u64 *sk_ntt_host, const u64 seed[8], u64 *ksk_host, u64 *seeds_host, std::unique_ptr<RelinKeys> *resident, bool sk_on_device)
{
    Enter g(this);
    if (!hp_.using_keyswitching) throw std::invalid_argument("parameters do not support key switching: the reference creates no relinearisation keys");
    const size_t n = hp_.n;
    const int K = hp_.K, nk = K - 1;
    if (!sk_on_device) check_key_residues(sk_ntt_host, K);
    const Blake2xbSeed master = master_seed(seed);
    std::vector<u64> seeds((size_t)nk * 8);
    for (int i = 0; i < nk; i++) blake2xb_stream_block(master, qs_seed_block((u64)i), seeds.data() + (size_t)i * 8);
    auto rk = std::make_unique<RelinKeys>();
    const size_t words = (size_t)nk * 2 * K * n;
    rk->data.alloc(words * sizeof(u64));
    std::vector<u64 *> a(nk);
    for (int i = 0; i < nk; i++) a[i] = rk->data.u() + ((size_t)i * 2 + 1) * K * n;
    TIER1_SLOTS();
    WITH_ARENA({
        const u64 *sk = sk_ntt_host;
        if (!sk_on_device) {
            u64 *staged = ws((size_t)K * n);
            HIP_CHECK(hipMemcpyAsync(staged, sk_ntt_host, (size_t)K * n * sizeof(u64), hipMemcpyHostToDevice, st_));
            sk = staged;
        }
        signed char *small = reinterpret_cast<signed char *>(ws((size_t)nk * n / 8));
        u64 *e = ws((size_t)nk * K * n);
        bool on_device = queue_seed_expand(K, nk, seeds.data(), a.data());
        if (!on_device) host_seed_expand(K, nk, seeds.data(), a.data());
        auto rest = [&] {
            { PROF(P_OTHER, 0); launch_sample_cbd(master, 0, small, n, nk, st_); }
            { PROF(P_OTHER, 0); launch_small_lift(dkey(), small, e, K, n, nk, st_); }
            d_ntt(e, (size_t)nk * K, map_ct(), K, false, data_primes_narrow_);
            { PROF(P_OTHER, 0); launch_rlk_finish(dkey(), K, sk, e, rk->data.u(), n, st_); }
            sync();
        };
        rest();
        if (on_device && seeds_overflowed(nk)) {                 // (seed_expand's fallback: the host redoes the public halves)
            host_seed_expand(K, nk, seeds.data(), a.data());
            rest();
        }
    });
    if (ksk_host) HIP_CHECK(hipMemcpy(ksk_host, rk->data.p(), words * sizeof(u64), hipMemcpyDeviceToHost));
    if (seeds_host) std::memcpy(seeds_host, seeds.data(), seeds.size() * sizeof(u64));
    if (resident) *resident = std::move(rk);
}

void Engine::query_create(const u64 *sk_ntt_host, const u64 seed[8], const uint32_t *bundle_indices, int nb, const u64 *values, bool values_on_device,
                          u64 *cts_dev, u64 *seeds_host, bool sk_on_device)
{
    Enter g(this);
    if (!has_psu_) throw std::logic_error("context was created without PSUParams");
    if (!hp_.batching) throw std::logic_error("plain_modulus does not support batching");
    if (nb <= 0) return;
    const size_t n = hp_.n;
    const int first = hp_.first_chain_idx, L = first + 1, tid = hp_.plain_id();
    std::vector<u32> exps(psu_.query_params.query_powers.begin(), psu_.query_params.query_powers.end());   // ascending (std::set)
    const int S = (int)exps.size(), count = nb * S;
    if ((size_t)nb * S > 65535) throw std::invalid_argument("more than 65535 ciphertexts in one call");
    for (int b = 0; b < nb; b++)
        if (bundle_indices[b] >= psu_.bundle_idx_count) throw std::invalid_argument("bundle index out of range");
    if (!sk_on_device) check_key_residues(sk_ntt_host, L);
    if (!values_on_device)
        for (size_t i = 0; i < (size_t)nb * n; i++)
            if (values[i] >= hp_.t) throw std::invalid_argument("slot value is not reduced modulo the plain modulus");
    const Blake2xbSeed master = master_seed(seed);
    std::vector<u64> seeds((size_t)count * 8);
    for (int c = 0; c < count; c++) blake2xb_stream_block(master, qs_seed_block(QS_KEY_OBJECTS + (u64)c), seeds.data() + (size_t)c * 8);
    std::vector<u64 *> c1(count);
    for (int c = 0; c < count; c++) c1[c] = cts_dev + ((size_t)c * 2 + 1) * L * n;
    u32 flags_host = 0;
    TIER1_SLOTS();
    WITH_ARENA({
        const u64 *sk = sk_ntt_host;
        if (!sk_on_device) {
            u64 *staged = ws((size_t)L * n);
            HIP_CHECK(hipMemcpyAsync(staged, sk_ntt_host, (size_t)L * n * sizeof(u64), hipMemcpyHostToDevice, st_));
            sk = staged;
        }
        const u64 *vals = values;
        if (!values_on_device) {
            u64 *staged = ws((size_t)nb * n);
            HIP_CHECK(hipMemcpyAsync(staged, values, (size_t)nb * n * sizeof(u64), hipMemcpyHostToDevice, st_));
            vals = staged;
        }
        u32 *flags = reinterpret_cast<u32 *>(ws(1));
        HIP_CHECK(hipMemsetAsync(flags, 0, sizeof(u64), st_));
        u64 *pt = ws((size_t)count * n);
        signed char *small = reinterpret_cast<signed char *>(ws((size_t)count * n / 8));
        u64 *v = ws((size_t)count * L * n);
        // PlaintextPowers + BatchEncoder::encode (plaintext_powers.cpp:41-46,51-99)
        { PROF(P_OTHER, 0); launch_plain_powers(vals, reinterpret_cast<const uint32_t *>(d_slot_map_.p()), upload_jobs(exps), S, make_mod(hp_.t), pt, n, nb, flags, st_); }
        d_ntt(pt, count, map_ct() + tid, 1, true, false);
        { PROF(P_OTHER, 0); launch_sample_cbd(master, QS_KEY_OBJECTS, small, n, count, st_); }
        // Encryptor::encrypt_symmetric: c1 from its public seed, v = c1 s, c0 = Delta(m) - e - v
        bool on_device = queue_seed_expand(L, count, seeds.data(), c1.data());
        if (!on_device) host_seed_expand(L, count, seeds.data(), c1.data());
        auto rest = [&] {
            std::vector<const u64 *> src((size_t)count * L);
            for (int c = 0; c < count; c++)
                for (int j = 0; j < L; j++) src[(size_t)c * L + j] = c1[c] + (size_t)j * n;
            bool nored = hp_.logn <= 14;                         // (limb j of c1 is a canonical residue of q_j: nothing to reduce)
            for (int j = 0; j < L && nored; j++) nored = ntt_gather_nored_ok(hp_.key_q[j], hp_.key_q[j], hp_.logn);
            { PROF(P_NTT_FWD, src.size());
              launch_ntt_gather(hp_.logn, upload_jobs(src), v, src.size(), tabs(), map_ct(), L, st_, nored, sw_.ntt_latency_limbs, data_primes_narrow_); }
            { PROF(P_OTHER, 0); launch_dyadic_plain(dlevel(first), v, sk, v, 1, n, count, 0, st_); }
            d_ntt(v, (size_t)count * L, map_ct(), L, true, data_primes_narrow_);
            { PROF(P_OTHER, 0); launch_enc_finish(dlevel(first), pt, v, small, cts_dev, n, count, st_); }
            HIP_CHECK(hipMemcpyAsync(&flags_host, flags, sizeof(u32), hipMemcpyDeviceToHost, st_));
            sync();
        };
        rest();
        if (on_device && seeds_overflowed(count)) {
            host_seed_expand(L, count, seeds.data(), c1.data());
            rest();
        }
    });
    if (flags_host & QS_FLAG_VALUE) throw std::invalid_argument("slot value is not reduced modulo the plain modulus");
    if (seeds_host) std::memcpy(seeds_host, seeds.data(), seeds.size() * sizeof(u64));
}

// ============================================================================ tier 2: BinBundle evaluation
// ---- the evaluation of one chunk of BinBundles, in pieces (eval_bundles below is the driver) ------------------------------
// What the pieces share: the call's arguments, the levels, the placement of the powers and the chunk's result / mask rows.
struct Engine::EvalCall {
    const Bundle *const *bundles; const Powers &pw; const RelinKeys *rk;
    const u64 *const *masks; bool masks_on_device; u64 *const *out_rows;
    size_t n; uint32_t l; int high, low; size_t Ll, Lh, Eh; u32 low_term_stride;
    std::vector<int> bslot;                                  // powers slot of every BinBundle of the call
    int c0 = 0;                                              // first BinBundle of the chunk being evaluated
    u64 *res = nullptr, *mask_d = nullptr;                   // the chunk's result rows / staged masks (when they are not the caller's)
    // powers are stored bundle-index major ([idx][power][2][L][n]): one index's powers are contiguous
    const u64 *low_ptr(uint32_t power, int b) const { return pw.low.u() + (((size_t)b * pw.n_low + (power - 1)) * 2) * Ll * n; }
    const u64 *hext_ptr(uint32_t i, int b) const { return pw.hext.u() + (((size_t)b * pw.n_high + (i - 1)) * 2) * Eh * n; }
    u64 *res_ptr(int i) const { return out_rows ? out_rows[c0 + i] : res + (size_t)i * 2 * n; }
    const u64 *mask_ptr(int i) const { return masks_on_device ? masks[c0 + i] : mask_d + (size_t)i * n; }
    const Bundle &bundle(int i) const { return *bundles[c0 + i]; }   // i: position in the chunk
    int slot(int i) const { return bslot[c0 + i]; }
};
// One batch: every Paterson-Stockmeyer BinBundle of the chunk, ordered by bundle index (the shared powers of
// one index then stay in the same L2).  (Cutting the batch into groups whose database scans overlap the previous
// group's VALU-bound tail on a second stream was built and measured in rounds 2 and 3, also with an LDS-DMA
// multiply-accumulate that leaves room for an NTT workgroup per CU: slower to level, the chip is power-bound.
// profiles/r03_eval_pipeline.txt; the code is in git history at 22dbbd1, engine.cpp:1600-1745.)
struct PsBatch {
    std::vector<int> ids;                               // positions in this chunk
    std::vector<int> nin, in_off;                       // inner polynomials per BinBundle, prefix offsets
    int Bs = 0, NI = 0;
    u64 *inner = nullptr, *ssum = nullptr, *vlast = nullptr, *term = nullptr, *cf = nullptr;
    std::vector<int> imap;                              // modulus of every limb polynomial of the merged block
    const int *imap_dev = nullptr;
    size_t n_vlast_side = 0;                            // limb polynomials at the end of the block that the side lane transforms back
    MacPlan mac;                                        // the multiply-accumulate launch, planned by ps_tables ...
    const MacJob *mac_jobs = nullptr;                   // ... its jobs on the device
    const TermJob *term_jobs = nullptr;                 // the i = 0 block's per-term products on the dropped limb (k_term_product)
    size_t n_term = 0; bool term_packed = false;
    // what the steps of ps_run hand on: the extended inner polynomials, the summed products, the deferred mod-down of the last
    // key switch (or nullptr), the side lane's i = 0 addend
    u64 *ext = nullptr, *result = nullptr, *ks_acc = nullptr, *i0_side = nullptr;
};

// BatchedPlaintextPolyn::eval (bin_bundle.cpp:106-174) for the BinBundles pl_ids of the chunk
void Engine::eval_plain(EvalCall &c, const std::vector<int> &pl_ids)
{
    const int Bp = (int)pl_ids.size();
    const int lvl = c.low;                                 // level of powers[1]
    const size_t Lv = lvl + 1;
    u64 *acc = ws((size_t)Bp * 2 * Lv * c.n);
    std::vector<MacStream> ms;
    std::vector<EpiJob> ej;
    for (int x = 0; x < Bp; x++) {
        const Bundle &b = c.bundle(pl_ids[x]);
        u64 *o = acc + (size_t)x * 2 * Lv * c.n;
        if (b.degree) ms.push_back(MacStream{ bundle_slot(b, false, 0, Lv * c.n), c.low_ptr(1, c.slot(pl_ids[x])), o, b.degree,
                                              bundle_stride(b, false, Lv * c.n), c.low_term_stride, (u32)(c.Ll * c.n), (u32)(Lv * c.n), 0, (u32)Lv,
                                              (u32)b.packed });   // :140-149
        else HIP_CHECK(hipMemsetAsync(o, 0, 2 * Lv * c.n * sizeof(u64), st_));
        ej.push_back(EpiJob{ o, nullptr, nullptr, b.a0.u(), c.mask_ptr(pl_ids[x]), c.res_ptr(pl_ids[x]) });
    }
    d_mac(plan_mac(ms, Lv, c.n));
    d_ntt_ct(acc, (size_t)Bp * 2, lvl, true);                                                 // :154
    // :159 add_plain(a_0), :162 add_plain(mask), :168-170 mod switch to the last level, :171 clear bits
    { PROFW(P_MODSWITCH, (size_t)Bp * c.n * (2 * Lv + 4)); launch_eval_epilogue(dlevel(0), lvl, upload_jobs(ej), Lv * c.n, hp_.irrelevant_bit_count, c.n, Bp, st_); }
}

// the sums of the pre-lifted coefficient-form plaintexts, sum_i lift(a_{i*h}) (.) C^{i*h} (bin_bundle.cpp:328-337), as MAC streams
void Engine::ps_cf_streams(const EvalCall &c, const PsBatch &g, std::vector<MacStream> &out)
{
    for (int x = 0; x < g.Bs; x++) {
        const Bundle &b = c.bundle(g.ids[x]);
        out.push_back(MacStream{ bundle_slot(b, true, 0, c.Lh * c.n), c.hext_ptr(1, c.slot(g.ids[x])), g.cf + (size_t)x * 2 * c.Lh * c.n, b.H,
                                 bundle_stride(b, true, c.Lh * c.n), (u32)((size_t)2 * c.Eh * c.n), (u32)(c.Eh * c.n), (u32)(c.Lh * c.n), 0, (u32)c.Lh,
                                 (u32)b.packed });
    }
}
// ... as a launch of their own on the current stream, where they did not join the main multiply-accumulate (CF_SIDE_LANE, CF_BEHIND_HIGH_READY)
void Engine::ps_cf_mac(const EvalCall &c, const PsBatch &g)
{
    std::vector<MacStream> cs;
    ps_cf_streams(c, g, cs);
    d_mac(plan_mac(cs, c.Lh, c.n));
}

// BatchedPlaintextPolyn::eval_patstock (bin_bundle.cpp:192-360) for the BinBundles ps_ids of the chunk: the batch, the plan
// (eval_plan.h, plan_eval: every form decision, enumerated on the CPU tier), the job tables (ps_tables) and the launch sequence (ps_run)
void Engine::eval_patstock(EvalCall &c, const std::vector<int> &ps_ids)
{
    if (c.low < c.high) throw std::logic_error("the low powers lie below the high powers");
    PsBatch g;
    g.ids = ps_ids;
    std::stable_sort(g.ids.begin(), g.ids.end(), [&](int a, int b) { return c.slot(a) < c.slot(b); });
    g.Bs = (int)g.ids.size();
    // inner polynomials i = 1..H (block H only if r > 0)                     :248-304
    g.nin.resize(g.Bs); g.in_off.resize(g.Bs);
    EvalState s{};
    for (int x = 0; x < g.Bs; x++) {
        const Bundle &b = c.bundle(g.ids[x]);
        g.nin[x] = (int)b.H - (b.r == 0 ? 1 : 0);
        g.in_off[x] = g.NI;
        g.NI += g.nin[x];
        s.max_terms = std::max(s.max_terms, g.nin[x]);
    }
    s.low = c.low; s.high = c.high;
    s.L = hlevel(c.high).L; s.nB = hlevel(c.high).nB;
    s.l = c.l; s.q_last = hlevel(c.low).q[c.Ll - 1];
    for (size_t j = 0; j < c.Lh; j++) s.q_widest = std::max(s.q_widest, hlevel(c.high).q[j]);
    s.Bs = g.Bs;
    s.high_in_flight = c.pw.high_async && c.pw.high_ready;
    s.eval_side = sw_.eval_side; s.prof_on = prof_on_; s.force_per_term = sw_.force_per_term; s.fuse_tensor = fuse_tensor_; s.fuse_tail = sw_.fuse_tail;
    s.lane2 = lanes_[2].st != nullptr; s.on_lane0 = cur_lane_ == 0;
    const EvalPlan plan = plan_eval(s);
    ps_tables(c, plan, g);
    ps_run(c, plan, g);
}

// phase A: workspace and the job array of the multiply-accumulate
void Engine::ps_tables(EvalCall &c, const EvalPlan &plan, PsBatch &g)
{
    const size_t n = c.n, Ll = c.Ll, Lh = c.Lh;
    const uint32_t l = c.l;
    const int Bs = g.Bs;
    const bool cf_here = plan.cf == CF_WITH_MAC;
    // Every dyadic multiply-accumulate of the evaluation reads only the query powers and the database, so
    // all of a group run as ONE launch, and their results share ONE inverse-NTT launch:
    //   inner [NI][2][Ll]   sum_j C^j (.) a_{i*h+j}                                  :258-264
    //   ssum  [Bs][2][Lh]   sum_j C^j (.) a_j on the limbs that survive the switch  (i = 0 block, fast form)
    //   vlast [Bs*l][2][1]  C^j (.) a_j on the dropped limb, per term               (i = 0 block, fast form)
    //   term  [Bs*l][2][Ll] C^j (.) a_j, per term                                   (i = 0 block, general form)
    //   cf    [Bs][2][Lh]   sum_i lift(a_{i*h}) (.) C^{i*h}                          :328-337 (exact)
    const size_t w_inner = (size_t)g.NI * 2 * Ll * n, w_ssum = plan.i0_fast ? (size_t)Bs * 2 * Lh * n : 0;
    const size_t w_vlast = plan.need_vlast ? (size_t)Bs * l * 2 * n : 0, w_term = plan.i0_fast ? 0 : (size_t)Bs * l * 2 * Ll * n;
    const size_t w_cf = (size_t)Bs * 2 * Lh * n;
    g.inner = ws(w_inner + w_ssum + w_vlast + w_term + (cf_here ? w_cf : 0));
    g.ssum = g.inner + w_inner; g.vlast = g.ssum + w_ssum; g.term = g.vlast + w_vlast;
    g.cf = cf_here ? g.term + w_term : nullptr;
    std::vector<MacStream> ms;
    auto map_push = [&](size_t polys, int first_limb, int limbs) {
        for (size_t p = 0; p < polys; p++) for (int j = 0; j < limbs; j++) g.imap.push_back(first_limb + j);
    };
    for (int x = 0; x < Bs; x++) {
        const Bundle &b = c.bundle(g.ids[x]);
        for (int i = 1; i <= g.nin[x]; i++) {
            const u32 cnt = (u32)i < b.H ? l : b.r;
            ms.push_back(MacStream{ bundle_slot(b, false, (size_t)i * l, Ll * n), c.low_ptr(1, c.slot(g.ids[x])),     // (slot i * l: bundle_layout.h)
                                    g.inner + ((size_t)g.in_off[x] + i - 1) * 2 * Ll * n, cnt,
                                    bundle_stride(b, false, Ll * n), c.low_term_stride, (u32)(Ll * n), (u32)(Ll * n), 0, (u32)Ll,
                                    (u32)b.packed });
        }
    }
    map_push((size_t)g.NI * 2, 0, (int)Ll);
    if (plan.raw_drop) for (int &v : g.imap) v |= NTT_MAP_RAW;     // consumed by the fused drop + extension only
    if (plan.i0_fast) {
        for (int x = 0; x < Bs; x++) {
            const Bundle &b = c.bundle(g.ids[x]);
            ms.push_back(MacStream{ bundle_slot(b, false, 0, Ll * n), c.low_ptr(1, c.slot(g.ids[x])), g.ssum + (size_t)x * 2 * Lh * n, l,
                                    bundle_stride(b, false, Ll * n), c.low_term_stride, (u32)(Ll * n), (u32)(Lh * n), 0, (u32)Lh,
                                    (u32)b.packed });
        }
        map_push((size_t)Bs * 2, 0, (int)Lh);
        if (plan.raw_i0) for (size_t x = g.imap.size() - (size_t)Bs * 2 * Lh; x < g.imap.size(); x++) g.imap[x] |= NTT_MAP_RAW;
    }
    std::vector<TermJob> tj;
    if (plan.need_vlast || !plan.i0_fast) {
        for (int x = 0; x < Bs; x++) {
            const Bundle &b = c.bundle(g.ids[x]);
            const int bs = c.slot(g.ids[x]);
            if (plan.i0_fast) {
                if (x == 0) g.term_packed = b.packed;
                else if (g.term_packed != (bool)b.packed) throw std::logic_error("BinBundles of one evaluation differ in their row format");
            }
            for (u32 j = 1; j <= l; j++) {
                if (plan.i0_fast)                            // the dropped limb of every term by itself: k_term_product (not k_mac chains of length one)
                    tj.push_back(TermJob{ bundle_slot(b, false, j - 1, Ll * n), c.low_ptr(j, bs), g.vlast + ((size_t)x * l + j - 1) * 2 * n });
                else
                    ms.push_back(MacStream{ bundle_slot(b, false, j - 1, Ll * n), c.low_ptr(j, bs),
                                            g.term + ((size_t)x * l + j - 1) * 2 * Ll * n, 1, bundle_stride(b, false, Ll * n), c.low_term_stride,
                                            (u32)(Ll * n), (u32)(Ll * n), 0, (u32)Ll, (u32)b.packed });
            }
        }
        if (plan.i0_fast) {
            map_push((size_t)Bs * l * 2, (int)Ll - 1, 1);
            if (plan.raw_i0) for (size_t x = g.imap.size() - (size_t)Bs * l * 2; x < g.imap.size(); x++) g.imap[x] |= NTT_MAP_RAW;
        } else map_push((size_t)Bs * l * 2, 0, (int)Ll);
    }
    if (plan.side_i0) g.n_vlast_side = (size_t)Bs * l * 2;
    if (cf_here) { ps_cf_streams(c, g, ms); map_push((size_t)Bs * 2, 0, (int)Lh); }
    g.mac = plan_mac(ms, Ll, n);
    g.mac_jobs = upload_jobs(g.mac.jobs);
    if (!tj.empty()) { g.term_jobs = upload_jobs(tj); g.n_term = tj.size(); }
}

// ---- phase B: the launch sequence.  The steps below, in the order ps_run takes them; each reads the call (c), the plan and what the
// steps before it left in the batch (g).
// the i = 0 block's per-term products on the dropped limb, on the current stream
void Engine::ps_term_product(const EvalCall &c, const PsBatch &g)
{
    PROF(P_MAC, (uint64_t)g.n_term * (g.term_packed ? packed_row_bits(hp_.key_q[c.Ll - 1]) : 64));
    launch_term_product(dlevel(c.low), g.term_jobs, g.n_term, c.n, (int)c.Ll - 1, (u32)(c.Ll * c.n), (u32)c.n, g.term_packed, st_);
}
// the i = 0 block's finish with one dropped limb (launch_i0_finish), on the current stream: one exact [2][Lh][n] addend per BinBundle
void Engine::ps_i0_finish(const EvalCall &c, const EvalPlan &plan, const PsBatch &g, u64 *i0)
{
    std::vector<I0Job> ij;
    for (int x = 0; x < g.Bs; x++)
        ij.push_back(I0Job{ g.ssum + (size_t)x * 2 * c.Lh * c.n, g.vlast + (size_t)x * c.l * 2 * c.n, i0 + (size_t)x * 2 * c.Lh * c.n, (int)c.l, 1 });
    PROFW(P_MODSWITCH, (size_t)g.Bs * c.n * (4 * c.Lh + 2 * c.l));
    launch_i0_finish(dlevel(c.low), upload_jobs(ij), c.n, g.Bs, st_, plan.raw_i0);
}

// 1. the multiply-accumulate (the level-`low` constants serve every limb: levels share their leading primes), the i = 0 block's term
// products and the merged inverse transform.  With I0_SIDE the term products and their transforms are left to the side lane:
// ev_fork_ marks the end of k_mac (the powers and the database are read-only from here on), ev_intt_ the end of the transforms.
void Engine::ps_mac(EvalCall &c, const EvalPlan &plan, PsBatch &g)
{
    d_mac(g.mac, g.mac_jobs);
    g.imap_dev = upload_jobs(g.imap);
    if (plan.side_i0) HIP_CHECK(hipEventRecord(ev_fork_, st_));
    else if (g.n_term) ps_term_product(c, g);
    d_ntt(g.inner, g.imap.size() - g.n_vlast_side, g.imap_dev, (int)g.imap.size(), true, false);    // :268,297,320,333
    if (plan.side_i0) HIP_CHECK(hipEventRecord(ev_intt_, st_));
}

// 2. the side lane (plan.side; why and what: eval_plan.h): the cf sums and, with I0_SIDE, the whole i = 0 block behind k_mac.  It starts
// behind the inverse transforms above, next to the drop / extension / transform launches (starting it behind the tensor-on-load
// transform instead, next to the finish and the key switch of the sums, measured level: profiles/r04_ab_eval_side.txt), and ends
// with ev_side_.
void Engine::ps_side(EvalCall &c, const EvalPlan &plan, PsBatch &g)
{
    g.cf = ws((size_t)g.Bs * 2 * c.Lh * c.n);
    if (plan.side_i0) g.i0_side = ws((size_t)g.Bs * 2 * c.Lh * c.n);
    else HIP_CHECK(hipEventRecord(ev_fork_, st_));
    switch_lane(2);
    struct Back { Engine *e; ~Back() { e->switch_lane(0); } } back{ this };
    HIP_CHECK(hipStreamWaitEvent(st_, ev_fork_, 0));
    if (plan.side_i0) {
        ps_term_product(c, g);
        d_ntt(g.vlast, g.n_vlast_side, g.imap_dev + (g.imap.size() - g.n_vlast_side), (int)g.n_vlast_side, true, false);
    }
    if (plan.wait_high_ready) HIP_CHECK(hipStreamWaitEvent(st_, c.pw.high_ready, 0));   // the cf sums read the high powers (second stream)
    ps_cf_mac(c, g);
    d_ntt_ct(g.cf, (size_t)g.Bs * 2, c.high, true);
    if (plan.side_i0) {
        HIP_CHECK(hipStreamWaitEvent(st_, ev_intt_, 0));     // the i = 0 finish also reads the sums the main stream transforms back
        ps_i0_finish(c, plan, g, g.i0_side);
    }
    HIP_CHECK(hipEventRecord(ev_side_, st_));
}

// 3. the inner polynomials: mod switch to the high level (:269,298), extension to q u Bsk and forward transform, ready for the
// ct x ct products.  A single drop is folded into the extension's pass (plan.fused_drop), which then reads RAW transforms.
void Engine::ps_drop_ext(EvalCall &c, const EvalPlan &plan, PsBatch &g)
{
    const size_t n = c.n;
    const int NI = g.NI;
    const LevelConstants &h = hlevel(c.high);
    g.ext = ws((size_t)NI * 2 * c.Eh * n);
    if (plan.fused_drop) {
        PROFW(P_BEHZ_EXT, (size_t)NI * 2 * n * (c.Ll + c.Eh));
        if (!launch_drop_behz_ext(dlevel(c.high), h.L, h.nB, g.inner, c.Ll * n, 1, g.ext, n, NI * 2, st_, plan.raw_drop))
            throw std::logic_error("the plan takes the fused drop + extension, the kernel table has none for this level");
    } else {
        u64 *innerh = g.inner;
        for (int lv = c.low; lv > c.high; lv--) {
            u64 *nxt = ws((size_t)NI * 2 * lv * n);
            { PROFW(P_MODSWITCH, (size_t)NI * 2 * n * (2 * lv + 1)); launch_modswitch(dlevel(lv), innerh, (size_t)2 * (lv + 1) * n, 2, nxt, n, NI, st_); }
            innerh = nxt;
        }
        { PROFW(P_BEHZ_EXT, (size_t)NI * 2 * n * (c.Lh + c.Eh)); launch_behz_ext(dlevel(c.high), h.L, h.nB, innerh, c.Lh * n, 1, g.ext, n, NI * 2, st_); }
    }
    d_ntt(g.ext, (size_t)NI * 2 * c.Eh, map_ext(c.high), (int)c.Eh, false, ext_primes_narrow_);
}

// 4. ct x ct with the high powers (:272,301) and the sum over i (:273,303), summed finish (plan.summed; why it is bit-identical:
// eval_plan.h): tensor, INTT, one finish per BinBundle.  With CF_BEHIND_HIGH_READY the cf sums join the inverse-NTT launch.
void Engine::ps_products_summed(EvalCall &c, const EvalPlan &plan, PsBatch &g)
{
    const size_t n = c.n, Lh = c.Lh, Eh = c.Eh, nBskh = Eh - Lh;
    const int Bs = g.Bs, NI = g.NI;
    const LevelConstants &h = hlevel(c.high);
    const bool late_cf = plan.cf == CF_BEHIND_HIGH_READY;
    g.result = ws((size_t)Bs * 3 * Lh * n);                                                     // :238-240
    u64 *dq = ws((size_t)NI * 3 * Lh * n + (size_t)Bs * 3 * nBskh * n + (late_cf ? (size_t)Bs * 2 * Lh * n : 0));
    u64 *bsum = dq + (size_t)NI * 3 * Lh * n;
    if (late_cf) {
        g.cf = bsum + (size_t)Bs * 3 * nBskh * n;
        ps_cf_mac(c, g);
    }
    std::vector<TensorSumJob> tj;
    std::vector<FinishSumJob> fj;
    std::vector<int> dmap;
    for (int x = 0; x < Bs; x++) {
        if (!g.nin[x]) { HIP_CHECK(hipMemsetAsync(g.result + (size_t)x * 3 * Lh * n, 0, 3 * Lh * n * sizeof(u64), st_)); continue; }
        const size_t job = (size_t)g.in_off[x];
        tj.push_back(TensorSumJob{ g.ext + job * 2 * Eh * n, c.hext_ptr(1, c.slot(g.ids[x])), dq + job * 3 * Lh * n,
                                   bsum + (size_t)x * 3 * nBskh * n, g.nin[x], 0 });
        fj.push_back(FinishSumJob{ dq + job * 3 * Lh * n, bsum + (size_t)x * 3 * nBskh * n, g.result + (size_t)x * 3 * Lh * n, g.nin[x], 0 });
    }
    // (the finish applies the inverse transform's twist itself where it is the unrolled kernel: raw output)
    const int rawf = fast_finish(c.high) ? NTT_MAP_RAW : 0;
    for (size_t p = 0; p < (size_t)NI * 3; p++) for (size_t j = 0; j < Lh; j++) dmap.push_back((int)j | rawf);
    for (size_t p = 0; p < (size_t)Bs * 3; p++) for (size_t i = 0; i < nBskh; i++) dmap.push_back(hp_.bsk_id(h.nB, (int)i) | rawf);
    if (late_cf) for (size_t p = 0; p < (size_t)Bs * 2; p++) for (size_t j = 0; j < Lh; j++) dmap.push_back((int)j);
    if (plan.fuse_tensor) {
        // per-term q limbs: product formed by the inverse transform's load; the Bsk sums (and cf) join the launch
        std::vector<TensorJob> pj;
        for (int x = 0; x < Bs; x++)
            for (int i = 0; i < g.nin[x]; i++) {
                const size_t job = (size_t)g.in_off[x] + i;
                pj.push_back(TensorJob{ g.ext + job * 2 * Eh * n, c.hext_ptr(1 + i, c.slot(g.ids[x])), dq + job * 3 * Lh * n });
            }
        // (only the Bsk limbs: four operand limbs per term in, three sums per BinBundle out)
        { PROFW(P_TENSOR, ((size_t)NI * 4 + (size_t)Bs * 3) * (Eh - Lh) * n); launch_tensor_sum(dlevel(c.high), (int)Eh, upload_jobs(tj), n, (int)tj.size(), (int)Lh, st_); }
        PROF(P_NTT_FUSED, dmap.size());
        launch_intt_tensor(hp_.logn, upload_jobs(pj), (int)pj.size(), (int)Lh, Eh * n, bsum, dmap.size() - pj.size() * 3 * Lh,
                           tabs(), upload_jobs(dmap), (int)dmap.size(), st_, sw_.ntt_latency_limbs);
    } else {
        { PROFW(P_TENSOR, ((size_t)NI * 4 * Eh + (size_t)NI * 3 * Lh + (size_t)Bs * 3 * (Eh - Lh)) * n); launch_tensor_sum(dlevel(c.high), (int)Eh, upload_jobs(tj), n, (int)tj.size(), 0, st_); }
        d_ntt(dq, dmap.size(), upload_jobs(dmap), (int)dmap.size(), true, false);
    }
    { PROFW(P_BEHZ_FINISH, ((size_t)NI * 3 * Lh + (size_t)Bs * 3 * (Eh - Lh) + (size_t)Bs * 3 * Lh) * n); launch_behz_finish_sum(dlevel(c.high), h.L, h.nB, upload_jobs(fj), n, (int)fj.size(), st_); }
}

// 5. the same with the per-term finish (the fallback: APSU_HE_EVAL_PER_TERM, more than four limbs, or terms * q_widest >= 2^63): every
// (BinBundle, block) product is finished (x t, floor, Bsk -> q) by its own threads, then the per-term results are summed per
// BinBundle (:273,303): the roundings stay per term (note N1)
void Engine::ps_products_per_term(EvalCall &c, const EvalPlan &plan, PsBatch &g)
{
    const size_t n = c.n, Lh = c.Lh, Eh = c.Eh;
    const int Bs = g.Bs, NI = g.NI;
    const LevelConstants &h = hlevel(c.high);
    g.result = ws((size_t)Bs * 3 * Lh * n);                                                     // :238-240
    if (plan.cf == CF_BEHIND_HIGH_READY) {
        g.cf = ws((size_t)Bs * 2 * Lh * n);
        ps_cf_mac(c, g);
        d_ntt_ct(g.cf, (size_t)Bs * 2, c.high, true);
    }
    u64 *dbuf = ws((size_t)NI * 3 * Eh * n);
    u64 *tbuf = ws((size_t)NI * 3 * Lh * n);
    std::vector<TensorJob> tj;                               // (one per inner polynomial: NI of them)
    std::vector<FinishJob> fj;
    std::vector<SumJob> sj;
    for (int x = 0; x < Bs; x++) {
        for (int i = 1; i <= g.nin[x]; i++) {
            const size_t job = (size_t)g.in_off[x] + i - 1;
            tj.push_back(TensorJob{ g.ext + job * 2 * Eh * n, c.hext_ptr(i, c.slot(g.ids[x])), dbuf + job * 3 * Eh * n });
            fj.push_back(FinishJob{ dbuf + job * 3 * Eh * n, tbuf + job * 3 * Lh * n, 1, 0 });
        }
        sj.push_back(SumJob{ tbuf + (size_t)g.in_off[x] * 3 * Lh * n, g.result + (size_t)x * 3 * Lh * n, g.nin[x], 0 });
    }
    if (plan.fuse_tensor) {
        PROF(P_NTT_FUSED, tj.size() * 3 * Eh);
        launch_intt_tensor(hp_.logn, upload_jobs(tj), (int)tj.size(), (int)Eh, Eh * n, nullptr, 0, tabs(), map_ext_fin(c.high), (int)Eh, st_, sw_.ntt_latency_limbs);
    } else {
        if (!tj.empty()) { PROF(P_TENSOR, 0); launch_tensor(dlevel(c.high), upload_jobs(tj), n, (int)tj.size(), st_); }
        d_ntt(dbuf, (size_t)NI * 3 * Eh, map_ext_fin(c.high), (int)Eh, true, ext_primes_narrow_);
    }
    { PROF(P_BEHZ_FINISH, 0); launch_behz_finish(dlevel(c.high), h.L, h.nB, upload_jobs(fj), false, n, (int)fj.size(), st_); }
    { PROF(P_BEHZ_FINISH, 0); launch_sum_jobs(dlevel(c.high), (int)Lh, upload_jobs(sj), 3, n, Bs, st_); }
}

// 7. the i = 0 block, reduced to one exact [2][Lh][n] addend per BinBundle
u64 *Engine::ps_i0(EvalCall &c, const EvalPlan &plan, PsBatch &g)
{
    const size_t n = c.n, Lh = c.Lh;
    const int Bs = g.Bs;
    if (plan.i0 == I0_SIDE) return g.i0_side;
    if (plan.i0 == I0_SSUM) return g.ssum;
    u64 *i0 = nullptr;
    if (plan.i0 == I0_FINISH_MAIN) {
        i0 = ws((size_t)Bs * 2 * Lh * n);
        ps_i0_finish(c, plan, g, i0);
    } else {
        u64 *termh = g.term;
        for (int lv = c.low; lv > c.high; lv--) {
            u64 *nxt = ws((size_t)Bs * c.l * 2 * lv * n);
            { PROFW(P_MODSWITCH, (size_t)Bs * c.l * 2 * n * (2 * lv + 1)); launch_modswitch(dlevel(lv), termh, (size_t)2 * (lv + 1) * n, 2, nxt, n, Bs * (int)c.l, st_); }
            termh = nxt;
        }
        i0 = ws((size_t)Bs * 2 * Lh * n);
        HIP_CHECK(hipMemsetAsync(i0, 0, (size_t)Bs * 2 * Lh * n * sizeof(u64), st_));
        { PROF(P_OTHER, 0); launch_add_many(dlevel(c.high), i0, 2 * Lh * n, termh, (int)c.l, 2, n, Bs, st_); }
    }
    return i0;
}

// 8. :340-343 the two exact addends, :345 add_plain(a_0), :346 add_plain(mask), :354-356 mod switch to the last
// level, :357 clear bits — one pass over the result
void Engine::ps_epilogue(EvalCall &c, PsBatch &g, const u64 *i0)
{
    const size_t n = c.n, Lh = c.Lh;
    std::vector<EpiJob> ej;
    for (int x = 0; x < g.Bs; x++)
        ej.push_back(EpiJob{ g.result + (size_t)x * 3 * Lh * n, i0 + (size_t)x * 2 * Lh * n, g.cf + (size_t)x * 2 * Lh * n,
                             c.bundle(g.ids[x]).a0.u(), c.mask_ptr(g.ids[x]), c.res_ptr(g.ids[x]),
                             g.ks_acc ? g.ks_acc + (size_t)x * 2 * (Lh + 1) * n : nullptr });
    PROFW(P_MODSWITCH, (size_t)g.Bs * n * (7 * Lh + 4 + (g.ks_acc ? 2 * (Lh + 1) : 0)));
    launch_eval_epilogue(dlevel(0), c.high, upload_jobs(ej), Lh * n, hp_.irrelevant_bit_count, n, g.Bs, st_, g.ks_acc ? dkey() : nullptr);
}

// the sequence, and which stream waits for which event (the side lane's own waits: ps_side)
void Engine::ps_run(EvalCall &c, const EvalPlan &plan, PsBatch &g)
{
    ps_mac(c, plan, g);
    if (plan.side) ps_side(c, plan, g);
    ps_drop_ext(c, plan, g);
    if (plan.wait_high_ready) HIP_CHECK(hipStreamWaitEvent(st_, c.pw.high_ready, 0));   // the products read the high powers (second stream)
    if (plan.summed) ps_products_summed(c, plan, g);
    else ps_products_per_term(c, plan, g);
    // 6. the last relinearisation (:308-310).  (round 6: its mod-down is performed by the epilogue kernel, on the way in: one launch fewer at
    // the end of every query, the updated (c0, c1) never go to memory; APSU_HE_FUSE_TAIL=0 keeps the launch)
    d_relinearize(g.result, 3 * c.Lh * c.n, g.Bs, *c.rk, c.high, nullptr, 0, plan.fuse_tail ? &g.ks_acc : nullptr);
    if (plan.side) HIP_CHECK(hipStreamWaitEvent(st_, ev_side_, 0));                     // cf sums (and the i = 0 addend) of the side lane
    ps_epilogue(c, g, ps_i0(c, plan, g));
}

void Engine::eval_bundles(const Bundle *const *bundles, int count, const Powers &pw, const RelinKeys *rk,
                          const u64 *const *masks, bool masks_on_device, u64 *out, bool out_on_device, u64 *const *out_rows)
{
    if (out_rows && !out_on_device) throw std::invalid_argument("out_rows are device-accessible destinations");
    Enter g(this);
    if (!has_psu_) throw std::logic_error("context was created without PSUParams");
    if (count <= 0) return;
    const size_t n = hp_.n;
    job_seq_base_ = 256;                                     // job-cache slots 256..: eval_bundles
    if (pw.low_async && pw.high_ready) HIP_CHECK(hipStreamWaitEvent(st_, pw.high_ready, 0));   // (pipelined walk: every power comes from the second stream)
    // the powers' last reader (see Powers::last_use): marked on the main stream when this call leaves, also by an exception --
    // kernels that read the powers may have been queued by then
    struct LastUse {
        Engine *e; const Powers &p;
        ~LastUse()
        {
            if (e->cur_lane_ != 0) e->switch_lane(0);
            if (!p.last_use && hipEventCreateWithFlags(&p.last_use, hipEventDisableTiming) != hipSuccess) { p.last_use = nullptr; p.last_use_set = false; return; }
            p.last_use_set = hipEventRecord(p.last_use, e->st_) == hipSuccess;
        }
    } last_use_mark{ this, pw };
    PhaseSpan ev_span;
    if (phase_on_) { ev_span.phase = PH_PROCESS_BIN_BUNDLE_CACHE; ev_span.a = phase_event(st_); }
    const uint32_t ps = psu_.query_params.ps_low_degree, l = ps;
    const int high = pw.high_level, low = pw.low_level;
    const size_t Ll = low + 1, Lh = high + 1;
    const size_t Eh = hlevel(high).L + hlevel(high).nB + 1;

    // validation mirrors bin_bundle.cpp:116-118,204-213 ("not enough ciphertext powers available")
    std::vector<int> bslot(count);
    bool any_ps = false;
    for (int i = 0; i < count; i++) {
        const Bundle &b = *bundles[i];
        bslot[i] = pw.slot_of(b.bundle_idx);
        if (bslot[i] < 0) throw std::invalid_argument("no ciphertext powers for this bundle index");
        if (b.use_ps) {
            any_ps = true;
            if (b.H > pw.n_high || l > pw.n_low) throw std::invalid_argument("not enough ciphertext powers available");
            if (b.pt_level != low) throw std::logic_error("plaintext level does not match the low powers");
        } else {
            if (b.degree > pw.n_low) throw std::invalid_argument("not enough ciphertext powers available");
            if (b.degree && b.pt_level != low) throw std::logic_error("plaintext level does not match the powers");
        }
    }
    // Without key switching the reference leaves eval_patstock's result unrelinearised (bin_bundle.cpp:238-240,308-310) and
    // the powers themselves may be longer than two polynomials: a path of its own
    if (pw.polys != (nks_ ? nks_S_ : 2u)) throw std::invalid_argument("ciphertext powers do not belong to this context");
    if (nks_ || result_polys_ > 2) {                        // every BinBundle of such a set: the rows are result_polys_ polynomials apart
        eval_bundles_nks(bundles, count, pw, masks, masks_on_device, out, out_on_device, out_rows);
        if (phase_on_ && ev_span.a) {
            ev_span.b = phase_event(st_);
            phase_spans_.push_back(ev_span);
            if (query_start_) { if (query_end_) phase_pool_.push_back(query_end_); query_end_ = phase_event(st_); }
        }
        return;
    }
    if (any_ps && !rk) throw std::invalid_argument("relinearization keys are required");

    EvalCall c{ bundles, pw, rk, masks, masks_on_device, out_rows, n, l, high, low, Ll, Lh, Eh, (u32)((size_t)2 * Ll * n), std::move(bslot) };

    // workspace budget -> chunk size
    size_t per_bundle_words = 0;
    for (int i = 0; i < count; i++) {
        const Bundle &b = *bundles[i];
        size_t w = 16 * n;
        if (b.use_ps) w += ((size_t)b.H * (2 * Ll + 2 * Lh + 2 * Eh + 3 * Eh) + (size_t)l * (2 * Ll + 2 * Lh) + 3 * Lh * (Lh + 4) + 8 * Lh) * n;
        else w += (size_t)(6 * Ll + 8) * n;
        per_bundle_words = std::max(per_bundle_words, w);
    }
    const size_t budget = sw_.eval_ws_bytes;
    int chunk = (int)std::max<size_t>(1, budget / (per_bundle_words * sizeof(u64)));
    chunk = std::min(chunk, count);

    bool synced = false;
    for (int c0 = 0; c0 < count; c0 += chunk) {
        const int B = std::min(chunk, count - c0);
        WITH_ARENA({
            // final [B][2][1][n]: written in place when the caller's buffer is on the device
            u64 *res = out_rows ? nullptr : (out_on_device ? out + (size_t)c0 * 2 * n : ws((size_t)B * 2 * n));
            u64 *mask_d = nullptr;
            if (!masks_on_device) {
                mask_d = ws((size_t)B * n);
                for (int i = 0; i < B; i++) H2D(mask_d + (size_t)i * n, masks[c0 + i], n);
            }
            c.c0 = c0; c.res = res; c.mask_d = mask_d;

            // split the chunk into Paterson-Stockmeyer and plain evaluations
            std::vector<int> ps_ids, pl_ids;
            for (int i = 0; i < B; i++) (bundles[c0 + i]->use_ps ? ps_ids : pl_ids).push_back(i);

            // ---------------------------------------------------------------- plain: bin_bundle.cpp:106-174
            if (!pl_ids.empty()) eval_plain(c, pl_ids);
            // ---------------------------------------------------------------- Paterson-Stockmeyer: bin_bundle.cpp:192-360
            if (!ps_ids.empty()) eval_patstock(c, ps_ids);
            if (!out_on_device) D2H(out + (size_t)c0 * 2 * n, res, (size_t)B * 2 * n);
            // device-resident masks and results: nothing of the caller's is read or written by the host, so the call may
            // return with the work queued (stream order protects the workspace, the job tables and the pooled powers)
            if (phase_on_ && c0 + B >= count) {                  // the last chunk closes the span (before any host wait)
                ev_span.b = phase_event(st_);
                phase_spans_.push_back(ev_span);
                if (query_start_) { if (query_end_) phase_pool_.push_back(query_end_); query_end_ = phase_event(st_); }
            }
            if (!(async_results_ && out_on_device && masks_on_device && !prof_on_)) { sync(); inflight_count_ = 0; synced = true; }
            else mark_inflight();
        });
    }
    if (synced) check_sources(pw);
}

// ============================================================================ no key switching: ciphertexts of any size
// One coefficient prime = SEALContext::using_keyswitching() false: Receiver::ComputePowers skips relinearize_inplace
// (receiver_osn.cpp:416,430-432) and eval_patstock does too (bin_bundle.cpp:308-310).  Every product then has
// size(a) + size(b) - 1 polynomials (Evaluator::bfv_multiply; Ciphertext::resize throws above SEAL_CIPHERTEXT_SIZE_MAX = 16),
// add_inplace takes the longer operand's size, multiply_plain / the transforms act on every polynomial.  There is one level
// (chain index 0, one limb), so no modulus switching.  Stored powers are zero-padded to a common even polynomial count
// (Powers::polys): the multiply-accumulate kernel handles a pair of polynomials per job, and a zero polynomial contributes
// zero to every sum, so only the SIZES are bookkeeping (power_size / result_size) -- the numbers are exact.
// Plain compositions of the per-polynomial kernels; nothing here is tuned (no shipped parameter set has products with one prime).

uint32_t Engine::power_size(uint32_t power) const
{
    if (!has_psu_) throw std::invalid_argument("context has no PSUParams");
    if (power >= nks_size_.size() || !nks_size_[power]) throw std::invalid_argument("power not available");
    return nks_size_[power];
}

// size of BatchedPlaintextPolyn::eval / eval_patstock's result for a BinBundle of this degree (bin_bundle.cpp:132-134 starts at
// size 2, :238-240 at size 3); values above CT_SIZE_MAX mean SEAL throws inside the evaluation
uint32_t Engine::result_size_for(uint32_t degree) const
{
    if (hp_.using_keyswitching) return 2;
    const uint32_t ps = psu_.query_params.ps_low_degree, h = ps + 1;
    auto sz = [&](uint32_t p) { return p < nks_size_.size() ? nks_size_[p] : 0u; };
    if (!(ps > 1 && ps < degree)) {                          // receiver_osn.cpp:520-522 -> eval
        uint32_t r = 2;
        for (uint32_t d = 1; d <= degree; d++) r = std::max(r, sz(d));
        return r;
    }
    const uint32_t H = degree / h, rem = degree % h;
    uint32_t r = 3, low_all = 2;
    for (uint32_t j = 1; j <= ps; j++) low_all = std::max(low_all, sz(j));
    for (uint32_t i = 1; i <= H; i++) {
        const uint32_t cnt = i < H ? ps : rem;
        if (!cnt) break;
        uint32_t s_in = 2;
        for (uint32_t j = 1; j <= cnt; j++) s_in = std::max(s_in, sz(j));
        r = std::max(r, s_in + sz(i * h) - 1);               // :272,301
    }
    r = std::max(r, low_all);                                // :314-324
    for (uint32_t i = 1; i <= H; i++) r = std::max(r, sz(i * h));    // :328-337
    return r;
}

uint32_t Engine::result_size(const Bundle &b) const
{
    if (!has_psu_) throw std::invalid_argument("context has no PSUParams");
    return result_size_for(b.degree);
}

void Engine::d_multiply_sized(const u64 *ea, int sa, const u64 *eb, int sb, u64 *out, int chain_idx)
{
    const size_t n = hp_.n, L = chain_idx + 1;
    const size_t E = hlevel(chain_idx).L + hlevel(chain_idx).nB + 1;
    const int so = sa + sb - 1, so3 = (so + 2) / 3 * 3;        // the finish kernels take polynomials three at a time
    u64 *d = ws((size_t)so3 * E * n), *o = ws((size_t)so3 * L * n);
    if (so3 > so) HIP_CHECK(hipMemsetAsync(d + (size_t)so * E * n, 0, (size_t)(so3 - so) * E * n * sizeof(u64), st_));
    std::vector<TensorConvJob> tj{ TensorConvJob{ ea, eb, d, sa, sb } };
    { PROF(P_TENSOR, 0); launch_tensor_conv(dlevel(chain_idx), upload_jobs(tj), n, 1, st_); }
    d_ntt(d, (size_t)so3 * E, map_ext_fin(chain_idx), (int)E, true, ext_primes_narrow_);
    std::vector<FinishJob> fj;
    for (int t = 0; t < so3 / 3; t++) fj.push_back(FinishJob{ d + (size_t)3 * t * E * n, o + (size_t)3 * t * L * n, 1, 0 });
    { PROF(P_BEHZ_FINISH, 0); launch_behz_finish(dlevel(chain_idx), hlevel(chain_idx).L, hlevel(chain_idx).nB, upload_jobs(fj), false, n, (int)fj.size(), st_); }
    D2D(out, o, (size_t)so * L * n);
}

void Engine::multiply_sized(const u64 *a, int sa, const u64 *b, int sb, u64 *out, int chain_idx)
{
    Enter g(this);
    TIER1_SLOTS();
    check_level(chain_idx);
    if (sa < 2 || sb < 2 || sa + sb - 1 > (int)CT_SIZE_MAX) throw std::invalid_argument("invalid size");      // Ciphertext::resize
    check_tier1_residues(a, (size_t)sa, chain_idx, "multiply_sized: operand holds a coefficient outside [0, q)");
    if (b != a) check_tier1_residues(b, (size_t)sb, chain_idx, "multiply_sized: operand holds a coefficient outside [0, q)");
    const size_t n = hp_.n, L = chain_idx + 1;
    const size_t E = hlevel(chain_idx).L + hlevel(chain_idx).nB + 1;
    const bool square = (a == b && sa == sb);
    WITH_ARENA({
        u64 *in = ws((size_t)(sa + (square ? 0 : sb)) * L * n);
        H2D(in, a, (size_t)sa * L * n);
        if (!square) H2D(in + (size_t)sa * L * n, b, (size_t)sb * L * n);
        const int np = sa + (square ? 0 : sb);
        u64 *ext = ws((size_t)np * E * n);
        { PROF(P_BEHZ_EXT, 0); launch_behz_ext(dlevel(chain_idx), hlevel(chain_idx).L, hlevel(chain_idx).nB, in, L * n, 1, ext, n, np, st_); }
        d_ntt(ext, (size_t)np * E, map_ext(chain_idx), (int)E, false, ext_primes_narrow_);
        u64 *o = ws((size_t)(sa + sb - 1) * L * n);
        d_multiply_sized(ext, sa, square ? ext : ext + (size_t)sa * E * n, sb, o, chain_idx);
        D2H(out, o, (size_t)(sa + sb - 1) * L * n);
        sync();
    });
}

std::unique_ptr<Powers> Engine::compute_powers_nks(const uint32_t *bundle_indices, int nb, const u64 *const *src, bool on_device)
{
    if (nks_oversize_)          // Evaluator::multiply -> Ciphertext::resize: std::invalid_argument("invalid size or poly_modulus_degree")
        throw std::invalid_argument("invalid size: a product of unrelinearized ciphertext powers exceeds SEAL's largest ciphertext");
    const Sched &s = sched_;
    const size_t n = hp_.n, S = nks_S_, P = s.slot_power.size();
    const size_t E = hlevel(0).L + hlevel(0).nB + 1;
    job_seq_base_ = 0;
    auto pw = std::make_unique<Powers>();
    if (++query_seq_ == 0) query_seq_ = 1;
    pw->seq = query_seq_;
    pw->nb = nb;
    pw->bundle_indices.assign(bundle_indices, bundle_indices + nb);
    pw->low_level = pw->high_level = 0;
    pw->n_low = (uint32_t)s.low_powers.size();
    pw->n_high = (uint32_t)s.high_powers.size();
    pw->polys = (uint32_t)S;
    counters_[C_POWERS_ALLOC]++;
    pw->low.alloc((size_t)pw->n_low * nb * S * n * sizeof(u64));
    if (pw->n_high) {
        pw->high.alloc((size_t)pw->n_high * nb * S * n * sizeof(u64));
        pw->hext.alloc((size_t)pw->n_high * nb * S * E * n * sizeof(u64));
    }
    PhaseSpan cp_span;
    if (phase_on_) {
        phase_close_query();
        cp_span.phase = PH_COMPUTE_POWERS;
        cp_span.a = phase_event(st_);
        query_start_ = phase_event(st_);
    }
    WITH_ARENA({
        if (cp_span.b) { phase_pool_.push_back(cp_span.b); cp_span.b = nullptr; }                  // a retry after arena growth
        // slot-major like the key-switching walk: [slot][bundle index][S polys]; coefficient form and extended + NTT form
        u64 *coef = ws(P * nb * S * n), *ext = ws(P * nb * S * E * n);
        HIP_CHECK(hipMemsetAsync(coef, 0, P * nb * S * n * sizeof(u64), st_));
        auto coef_ptr = [&](int slot, int b) { return coef + ((size_t)slot * nb + b) * S * n; };
        auto ext_ptr = [&](int slot, int b) { return ext + ((size_t)slot * nb + b) * S * E * n; };
        int si = 0;
        std::vector<CtJob> chk;
        for (auto &kv : dag_.nodes()) {                                                            // receiver_osn.cpp:304-317
            if (!kv.second.is_source()) continue;
            for (int b = 0; b < nb; b++) {
                const u64 *sp = src[(size_t)b * dag_.source_count() + si];
                if (on_device) D2D(coef_ptr(s.slot_of[kv.first], b), sp, 2 * n);
                else H2D(coef_ptr(s.slot_of[kv.first], b), sp, 2 * n);
                chk.push_back(CtJob{ coef_ptr(s.slot_of[kv.first], b), coef_ptr(s.slot_of[kv.first], b) });
            }
            si++;
        }
        // the sources against their (single) prime, in place: the same report as on the key-switching path (round 6)
        launch_copy_sources(upload_jobs(chk), 2 * n, (int)chk.size(), dlevel(0), 1, n, bad_source_ + query_seq_ % BAD_SLOTS, query_seq_, st_);
        // BEHZ extension + NTT of every polynomial of the slots [s0, s1) (zero padding extends to zero)
        auto extend = [&](int s0, int s1) {
            if (s1 <= s0) return;
            { PROF(P_BEHZ_EXT, 0); launch_behz_ext(dlevel(0), hlevel(0).L, hlevel(0).nB, coef_ptr(s0, 0), S * n, (int)S, ext_ptr(s0, 0), n, (s1 - s0) * nb, st_); }
            d_ntt(ext_ptr(s0, 0), (size_t)(s1 - s0) * nb * S * E, map_ext(0), (int)E, false, ext_primes_narrow_);
        };
        extend(s.levels[0].s0, s.levels[0].s1);
        for (size_t d = 1; d < s.levels.size(); d++) {
            const size_t mark = arena_off_;
            for (const auto &nd : s.nodes) {                                                       // :418-433, one product per node and index
                if (nd[0] < s.levels[d].s0 || nd[0] >= s.levels[d].s1) continue;
                const int sa = (int)nks_size_[s.slot_power[nd[1]]], sb = (int)nks_size_[s.slot_power[nd[2]]];
                for (int b = 0; b < nb; b++) {
                    d_multiply_sized(ext_ptr(nd[1], b), sa, ext_ptr(nd[2], b), sb, coef_ptr(nd[0], b), 0);
                    arena_off_ = mark;                                                             // stream order makes the reuse safe
                }
            }
            extend(s.levels[d].s0, s.levels[d].s1);
        }
        // :458-487: no level below the first one; low powers (all of them without Paterson-Stockmeyer) go to NTT form
        for (size_t i = 0; i < s.low_powers.size(); i++)
            for (int b = 0; b < nb; b++)
                D2D(pw->low.u() + ((size_t)b * pw->n_low + i) * S * n, coef_ptr(s.slot_of[s.low_powers[i]], b), S * n);
        d_ntt_ct(pw->low.u(), (size_t)pw->n_low * nb * S, 0, false);
        for (size_t i = 0; i < s.high_powers.size(); i++)
            for (int b = 0; b < nb; b++) {
                D2D(pw->high.u() + ((size_t)b * pw->n_high + i) * S * n, coef_ptr(s.slot_of[s.high_powers[i]], b), S * n);
                D2D(pw->hext.u() + ((size_t)b * pw->n_high + i) * S * E * n, ext_ptr(s.slot_of[s.high_powers[i]], b), S * E * n);
            }
        if (phase_on_ && cp_span.a) cp_span.b = phase_event(st_);
        sync();                                              // the workspace is reused by the next call; nothing here is latency-critical
    });
    if (phase_on_ && cp_span.a && cp_span.b) phase_spans_.push_back(cp_span);
    pw->last_use_set = false;                               // (the path synchronises; kept for the pool's bookkeeping)
    check_sources(*pw);                                      // this path has just waited: the report comes from the call that took the sources
    return pw;
}

void Engine::eval_bundles_nks(const Bundle *const *bundles, int count, const Powers &pw, const u64 *const *masks, bool masks_on_device,
                              u64 *out, bool out_on_device, u64 *const *out_rows)
{
    const size_t n = hp_.n, S = pw.polys, R = result_polys_;
    const size_t E = hlevel(0).L + hlevel(0).nB + 1;
    const uint32_t l = psu_.query_params.ps_low_degree, h = l + 1;
    auto even = [](uint32_t v) { return (v + 1) & ~1u; };
    auto sz = [&](uint32_t p) { return nks_size_[p]; };
    std::vector<uint32_t> rs(count);
    for (int i = 0; i < count; i++) {
        rs[i] = result_size_for(bundles[i]->degree);
        if (rs[i] > CT_SIZE_MAX)                             // Evaluator::multiply inside eval_patstock would throw
            throw std::invalid_argument("invalid size: a Paterson-Stockmeyer product exceeds SEAL's largest ciphertext");
    }
    WITH_ARENA({
        u64 *res = out_rows ? nullptr : (out_on_device ? out : ws((size_t)count * R * n));
        auto res_ptr = [&](int i) { return out_rows ? out_rows[i] : res + (size_t)i * R * n; };
        u64 *mask_d = nullptr;
        if (!masks_on_device) {
            mask_d = ws((size_t)count * n);
            for (int i = 0; i < count; i++) H2D(mask_d + (size_t)i * n, masks[i], n);
        }
        auto low_ptr = [&](int b) { return pw.low.u() + (size_t)b * pw.n_low * S * n; };            // power 1 of bundle-index slot b
        auto hext_ptr = [&](uint32_t i, int b) { return pw.hext.u() + ((size_t)b * pw.n_high + (i - 1)) * S * E * n; };
        const size_t base_mark = arena_off_;
        for (int x = 0; x < count; x++) {
            arena_off_ = base_mark;                                                                 // stream order makes the reuse safe
            const Bundle &b = *bundles[x];
            const int bs = pw.slot_of(b.bundle_idx);
            const uint32_t RS = even(rs[x]);
            u64 *result = ws((size_t)RS * n);                                                       // coefficient form
            std::vector<MacStream> ms;
            // every stream: pairs of polynomials (2k, 2k+1) of the powers, terms 1..cnt of a run of NTT-form plaintexts
            auto low_streams = [&](const u64 *pt, u32 cnt, uint32_t polys, u64 *acc) {
                for (uint32_t pp = 0; pp < even(polys) / 2; pp++)
                    ms.push_back(MacStream{ pt, low_ptr(bs) + (size_t)pp * 2 * n, acc + (size_t)pp * 2 * n, cnt, (u32)n, (u32)(S * n), (u32)n, (u32)n, 0, 1 });
            };
            auto size_upto = [&](uint32_t cnt) { uint32_t v = 2; for (uint32_t j = 1; j <= cnt; j++) v = std::max(v, sz(j)); return v; };
            if (!b.use_ps) {                                                                        // bin_bundle.cpp:106-174
                if (b.degree) {
                    low_streams(b.ntt.u(), b.degree, rs[x], result);                                // :140-149
                    d_mac(plan_mac(ms, 1, n));
                    d_ntt_ct(result, RS, 0, true);                                                  // :154
                } else {
                    HIP_CHECK(hipMemsetAsync(result, 0, (size_t)RS * n * sizeof(u64), st_));
                }
            } else {                                                                                // bin_bundle.cpp:192-360
                const uint32_t H = b.H, nin = H - (b.r == 0 ? 1 : 0);
                // one multiply-accumulate launch and one inverse transform for: the inner polynomials (:258-264,287-293), the
                // i = 0 block sum_j C^j a_j (:314-324; the sum of the terms' inverse transforms is the transform of the sum,
                // and there is no modulus switch to round per term), and sum_i C^{ih} a_{ih} (:328-337, exact)
                std::vector<uint32_t> s_in(nin + 1, 2);
                std::vector<u64 *> inner(nin + 1, nullptr);
                size_t words = 0;
                for (uint32_t i = 1; i <= nin; i++) { s_in[i] = size_upto(i < H ? l : b.r); words += (size_t)even(s_in[i]) * n; }
                const uint32_t s_low = size_upto(l);
                uint32_t s_high = 2;
                for (uint32_t i = 1; i <= H; i++) s_high = std::max(s_high, sz(i * h));
                u64 *blk = ws(words + (size_t)(even(s_low) + even(s_high)) * n);
                u64 *cur = blk;
                for (uint32_t i = 1; i <= nin; i++) {
                    inner[i] = cur;
                    low_streams(b.ntt.u() + (size_t)i * l * n, i < H ? l : b.r, s_in[i], cur);                // (slot i * l: bundle_layout.h)
                    cur += (size_t)even(s_in[i]) * n;
                }
                u64 *lowsum = cur, *cf = cur + (size_t)even(s_low) * n;
                low_streams(b.ntt.u(), l, s_low, lowsum);
                for (uint32_t pp = 0; pp < even(s_high) / 2; pp++)
                    ms.push_back(MacStream{ b.lifted.u(), hext_ptr(1, bs) + (size_t)pp * 2 * E * n, cf + (size_t)pp * 2 * n, H, (u32)n,
                                            (u32)(S * E * n), (u32)(E * n), (u32)n, 0, 1 });
                d_mac(plan_mac(ms, 1, n));
                d_ntt_ct(blk, (words / n) + even(s_low) + even(s_high), 0, true);                   // :268,297,321 and the product's transform
                HIP_CHECK(hipMemsetAsync(result, 0, (size_t)RS * n * sizeof(u64), st_));            // :238-240
                for (uint32_t i = 1; i <= nin; i++) {                                               // :272-273,301-303
                    const size_t mark = arena_off_;
                    const int sa = (int)s_in[i], sb = (int)sz(i * h), so = sa + sb - 1;
                    u64 *iext = ws((size_t)sa * E * n), *prod = ws((size_t)so * n);
                    { PROF(P_BEHZ_EXT, 0); launch_behz_ext(dlevel(0), hlevel(0).L, hlevel(0).nB, inner[i], n, 1, iext, n, sa, st_); }
                    d_ntt(iext, (size_t)sa * E, map_ext(0), (int)E, false, ext_primes_narrow_);
                    d_multiply_sized(iext, sa, hext_ptr(i, bs), sb, prod, 0);
                    { PROF(P_OTHER, 0); launch_add(dlevel(0), result, prod, so, n, 1, st_); }
                    arena_off_ = mark;
                }
                { PROF(P_OTHER, 0); launch_add(dlevel(0), result, lowsum, (int)s_low, n, 1, st_); }
                { PROF(P_OTHER, 0); launch_add(dlevel(0), result, cf, (int)s_high, n, 1, st_); }
            }
            // :159-171 / :345-357: add_plain(a_0), add_plain(mask) on the first polynomial; one level, so no modulus switch;
            // clear the irrelevant bits of every polynomial.  Row layout: rs[x] polynomials, zeros up to R.
            u64 *row = res_ptr(x);
            const u64 *mk = masks_on_device ? masks[x] : mask_d + (size_t)x * n;
            std::vector<EpiJob> ej{ EpiJob{ result, nullptr, nullptr, b.a0.u(), mk, row } };
            { PROF(P_MODSWITCH, 0); launch_eval_epilogue(dlevel(0), 0, upload_jobs(ej), n, hp_.irrelevant_bit_count, n, 1, st_); }
            if (rs[x] > 2) {
                D2D(row + 2 * n, result + 2 * n, (size_t)(rs[x] - 2) * n);
                { PROF(P_OTHER, 0); launch_clear_bits(row + 2 * n, (size_t)(rs[x] - 2) * n, hp_.irrelevant_bit_count, st_); }
            }
            if (R > rs[x]) HIP_CHECK(hipMemsetAsync(row + (size_t)rs[x] * n, 0, (R - rs[x]) * n * sizeof(u64), st_));
        }
        if (!out_rows && !out_on_device) D2H(out, res, (size_t)count * R * n);
        sync();
        inflight_count_ = 0;
    });
}

} // namespace apsu_he
