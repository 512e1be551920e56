// What the Engine's three translation units share and nobody else sees: engine.cpp (contexts, tier 1, ComputePowers, the evaluation,
// the querier's side), engine_bundles.cpp (what makes, stores and converts a BinBundle: upload, build, encode and decode, images) and
// engine_db.cpp (the calls on a resident database: update, lookup, bins, merge and compaction, export, plaintext evaluation, self-test).
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

// `count` objects of type T from the arena (whole 64-bit words, rounded up) and `extra` words behind them
template <class T> T *Engine::ws_as(size_t count, size_t extra) { return reinterpret_cast<T *>(ws((count * sizeof(T) + 7) / 8 + extra)); }

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
