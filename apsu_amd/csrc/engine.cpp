// See engine.h.  Host orchestration of the HIP kernels; mirrors, step for step,
//   Receiver::ComputePowers                 receiver/apsu/receiver_osn.cpp:395-488     (engine_powers.cpp)
//   BatchedPlaintextPolyn::eval             receiver/apsu/bin_bundle.cpp:106-174       (engine_eval.cpp)
//   BatchedPlaintextPolyn::eval_patstock    receiver/apsu/bin_bundle.cpp:192-360       (engine_eval.cpp)
// Exact (rounding-free) steps are batched / re-associated freely; every rounding step
// (drop-limb, BEHZ floor, key-switch mod-down) is applied per term exactly where the reference
// applies it (SURVEY.md §2.4 note N1), so results are bit-identical to the CPU path.
// This unit: the context itself -- construction, waits and source checks, lanes, profiling and phase timers, the arena, the device
// building blocks every other unit launches through, and tier 1.
#include "engine_impl.h"

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
    if (sw_.seed_rej_cap < 1 || sw_.seed_rej_cap > SEED_REJ_CAP) throw std::invalid_argument("APSU_HE_SEED_REJ_CAP outside 1 .. 8192");
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
        // the walks and the polynomial counts are pure functions of the PowersDag (powers_sched.h)
        const uint32_t ps = psu_.query_params.ps_low_degree;
        PowersScheds scheds = powers_scheds(dag_, ps);
        split_ok_ = scheds.split_ok;
        sched_ = std::move(scheds.all); sched_low_ = std::move(scheds.low); sched_high_ = std::move(scheds.high);
        sizes_ = power_sizes(sched_, hp_.using_keyswitching, dag_.depth());
        result_polys_ = apsu_he::result_polys(sizes_, ps, hp_.using_keyswitching, psu_.table_params.max_items_per_bin);
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

// ============================================================================ arena (ws and upload_jobs: engine_impl.h)
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

} // namespace apsu_he
