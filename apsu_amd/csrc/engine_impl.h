// What the Engine's translation units share and nobody else sees.  engine.cpp: the context (construction, waits, lanes, profiling and
// phase timers, the arena, the device building blocks, tier 1); engine_powers.cpp: ComputePowers; engine_eval.cpp: the BinBundle
// evaluation; engine_query.cpp: seeded expansion, masks and packing, the querier's side; engine_nks.cpp: both paths without key
// switching; engine_bundles.cpp: what makes, stores and converts a BinBundle (upload, build, encode and decode, images); engine_db.cpp: the
// calls on a resident database (update, lookup, bins, merge and compaction, export, plaintext evaluation, self-test); engine_cuckoo.cpp and
// the engine_*_steps.cpp test hooks.  The arena's allocator and the job-table upload are defined HERE, not in a unit: a launch path
// then crosses no unit boundary for them.
#pragma once
#include "engine.h"

#include <algorithm>
#include <cstring>
#include <stdexcept>

namespace apsu_he {

void throw_hip(hipError_t e, const char *file, int line);
#define HIP_CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw_hip(e_, __FILE__, __LINE__); } while (0)

struct ArenaOverflow { size_t need; };                           // thrown by Engine::ws, caught by with_arena

// Every public entry point serialises on the context and runs with the context's device current: HIP's current
// device is per host thread, and the reference calls the Evaluator from a thread pool (receiver_osn.cpp:334-364),
// so a worker thread may arrive with another device selected (several contexts on different GPUs in one process).
struct Engine::Enter {
    std::lock_guard<std::mutex> lock;
    int prev = -1;
    explicit Enter(Engine *e) : lock(e->mu_)
    {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != e->device_) { prev = cur; HIP_CHECK(hipSetDevice(e->device_)); }
    }
    ~Enter() { if (prev >= 0) (void)hipSetDevice(prev); }
};

struct ProfScope {
    Engine *e;
    ProfScope(Engine *e_, int kind, uint64_t units) : e(e_) { e->prof_begin(kind, units); }
    ~ProfScope() { e->prof_end(); }
};
#define PROF(kind, units) ProfScope prof_scope_(this, kind, units)
// element-wise classes: units = ALGORITHMIC bytes of the launch (compulsory operand reads + result writes, 8 bytes per word;
// level constants and the relinearisation keys -- shared by every coefficient, cache-resident -- not counted)
#define PROFW(kind, words) ProfScope prof_scope_(this, kind, (uint64_t)(words) * 8)

// run `fn` with the arena, growing it and retrying when the bump allocator overflows
template <class F> static void with_arena(Engine *e, F &&fn, void (Engine::*reset)(size_t))
{
    size_t need = 0;
    for (int attempt = 0; attempt < 40; attempt++) {
        (e->*reset)(need);
        try { fn(); return; }
        catch (const ArenaOverflow &o) { need = std::max(o.need * 2, need); }
    }
    throw std::runtime_error("workspace arena could not be sized");
}
struct EngineAccess {
    template <class F> static void run(Engine *e, F &&fn) { with_arena(e, fn, &Engine::ws_reset); }
};
#define WITH_ARENA(...) EngineAccess::run(this, [&]() __VA_ARGS__)
#define TIER1_SLOTS() job_seq_base_ = 512

// ---- the arena and the job tables: defined here so that every unit's launch path allocates and uploads without leaving its unit
inline u64 *Engine::ws(size_t words)
{
    size_t bytes = (words * sizeof(u64) + 255) & ~(size_t)255;
    if (arena_off_ + bytes > arena_.bytes()) { overflow_lane_ = cur_lane_; throw ArenaOverflow{ arena_off_ + bytes }; }
    u64 *p = reinterpret_cast<u64 *>(static_cast<char *>(arena_.p()) + arena_off_);
    arena_off_ += bytes;
    return p;
}

// `count` objects of type T from the arena (whole 64-bit words, rounded up) and `extra` words behind them
template <class T> T *Engine::ws_as(size_t count, size_t extra) { return reinterpret_cast<T *>(ws((count * sizeof(T) + 7) / 8 + extra)); }

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

// The ComputePowers phase span around a walk (compute_powers, compute_powers_nks): opened on the current stream together with the
// RunQuery span, closed when body(span), which runs inside WITH_ARENA, has stamped span.b (and span.b2 on a second stream).  A retry
// after arena growth queues the walk again: the stamps of the attempt before go back to the pool first.
template <class F> void Engine::with_powers_span(F &&body)
{
    PhaseSpan span;
    if (phase_on_) {
        phase_close_query();
        span.phase = PH_COMPUTE_POWERS;
        span.a = phase_event(st_);
        query_start_ = phase_event(st_);
    }
    WITH_ARENA({
        for (hipEvent_t *e : { &span.b, &span.b2 }) if (*e) { phase_pool_.push_back(*e); *e = nullptr; }
        body(span);
    });
    if (phase_on_ && span.a && span.b) phase_spans_.push_back(span);
}

// Tier-1 operands are host pointers by default; with apsu_he_set_tier1_on_device they are device (or page-locked) memory and the
// calls only queue their work -- unified addressing lets one copy kind serve both
#define H2D(dst, src, words) HIP_CHECK(hipMemcpyAsync(dst, src, (words) * sizeof(u64), tier1_device_ ? hipMemcpyDefault : hipMemcpyHostToDevice, st_))
#define D2H(dst, src, words) HIP_CHECK(hipMemcpyAsync(dst, src, (words) * sizeof(u64), tier1_device_ ? hipMemcpyDefault : hipMemcpyDeviceToHost, st_))
#define D2D(dst, src, words) HIP_CHECK(hipMemcpyAsync(dst, src, (words) * sizeof(u64), hipMemcpyDeviceToDevice, st_))

// Caller data mod t: every v[i] < t, else std::invalid_argument naming the first one that is not -- name(i, v[i]) says what it is
inline std::string not_reduced(const std::string &subject) { return subject + " is not reduced modulo plain_modulus"; }
template <class Name> void check_reduced(const u64 *v, size_t count, u64 t, Name name)
{
    for (size_t i = 0; i < count; i++)
        if (v[i] >= t) throw std::invalid_argument(not_reduced(name(i, v[i])));
}
inline std::string field_element(size_t, u64) { return "field element"; }

inline bool is_monomial(const u64 *pt, size_t count)           // SEAL's multiply_plain takes a monomial without lifting it
{
    size_t nz = 0;
    for (size_t k = 0; k < count && nz < 2; k++) nz += pt[k] != 0;
    return nz == 1;
}

} // namespace apsu_he
