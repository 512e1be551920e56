// The Engine's ComputePowers (receiver/apsu/receiver_osn.cpp:395-488): walks over the schedules of powers_sched.h, ordered by the
// plan of sched_policy.h.  The schedules themselves are made at creation (engine.cpp); nothing in here decides a slot or a level.
#include "engine_impl.h"
#include "sched_policy.h"

namespace apsu_he {

// One walk over a (sub)schedule of the PowersDag on the current lane: sources (dag_sources), the level-synchronous products
// (dag_level(d), d = 1 ..), and the final per-power conversions (dag_outputs) (receiver_osn.cpp:395-488).
// The steps of one walk must run in order on one lane; DagRun carries the walk's buffers between them, so two walks
// (the halves of a split DAG) can be interleaved level by level on two lanes.
struct Engine::DagRun {
    const PowersSched &s; int nb; size_t n, Lf, Ef, slot_w;       // slot_w: (c0, c1, c2 scratch) per power and bundle index
    u64 *pwf = nullptr, *ext = nullptr, *dbuf = nullptr; size_t arena_mark = 0; int ext_done = -1;   // ext_done: level whose parents are already extended
    DagRun(const Engine &e, const PowersSched &s_, int nb_)
        : s(s_), nb(nb_), n(e.hp_.n), Lf(e.hp_.first_chain_idx + 1),
          Ef(e.dlevel(e.hp_.first_chain_idx) ? (size_t)(e.hlevel(e.hp_.first_chain_idx).L + e.hlevel(e.hp_.first_chain_idx).nB + 1) : 0), slot_w(3 * Lf * n) {}
    u64 *slot_ptr(int slot, int b) const { return pwf + ((size_t)slot * nb + b) * slot_w; }
    u64 *ext_ptr(int slot, int b) const { return ext + ((size_t)slot * nb + b) * 2 * Ef * n; }
};

// workspace + sources (receiver_osn.cpp:304-317)
void Engine::dag_sources(DagRun &run, const u64 *const *src, bool on_device)
{
    const PowersSched &s = run.s;
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
    const PowersSched &s = run.s;
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
    const PowersSched &s = run.s;
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
void Engine::dag_walk(const PowersSched &s, int nb, const u64 *const *src, bool on_device, const RelinKeys *rk, Powers &pw)
{
    DagRun r(*this, s, nb);
    dag_sources(r, src, on_device);
    for (size_t d = 1; d < s.levels.size(); d++) dag_level(r, d, rk);
    dag_outputs(r, pw, true, true);
}

// the header of a query's Powers: a new sequence number, the bundle indices, the levels and the counts of the whole DAG's schedule
void Engine::powers_header(Powers &pw, const uint32_t *bundle_indices, int nb, int low_level, int high_level)
{
    if (++query_seq_ == 0) query_seq_ = 1;                   // (0 = "never computed")
    pw.seq = query_seq_;
    pw.nb = nb;
    pw.bundle_indices.assign(bundle_indices, bundle_indices + nb);
    pw.low_level = low_level;
    pw.high_level = high_level;
    pw.n_low = (uint32_t)sched_.low_powers.size();
    pw.n_high = (uint32_t)sched_.high_powers.size();
    pw.polys = sizes_.stored;
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
    if (sizes_.products) return compute_powers_nks(bundle_indices, nb, src, on_device);
    const PowersSched &s = sched_;
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
    powers_header(*pw, bundle_indices, nb, low_target, high);
    if (!recycled) {
        counters_[C_POWERS_ALLOC]++;
        pw->low.alloc(need_low);
        if (pw->n_high) {
            pw->high.alloc(need_high);
            pw->hext.alloc(need_hext);
        }
    }

    struct LaneGuard { Engine *e; ~LaneGuard() { e->switch_lane(0); } } lane_guard{ this };
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
    with_powers_span([&](PhaseSpan &cp_span) {
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
    const PowerPlace at = power_place(psu_.query_params.ps_low_degree, power, pw.n_low, pw.n_high);
    const bool low = at.low;
    const int lvl = low ? pw.low_level : pw.high_level;
    const size_t words = (size_t)power_size(power) * (lvl + 1) * hp_.n;               // the stored slot may be zero-padded beyond that
    if (capacity_words < words) throw std::invalid_argument("output buffer too small");
    sync();
    check_sources(pw);
    const u64 *src = (low ? pw.low.u() : pw.high.u()) + ((size_t)b * (low ? pw.n_low : pw.n_high) + at.idx) * pw.polys * (lvl + 1) * hp_.n;
    HIP_CHECK(hipMemcpy(out, src, words * sizeof(u64), hipMemcpyDeviceToHost));
    if (chain_idx) *chain_idx = lvl;
    if (is_ntt) *is_ntt = low ? 1 : 0;
}

} // namespace apsu_he
