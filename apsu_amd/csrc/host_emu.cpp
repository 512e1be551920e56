// CPU emulation of the product's host logic, of one NTT workgroup and of the multiply-accumulate family, for the no-GPU test tier.
// The NTT emulation executes the SAME pass functions (ntt_core.h) the gfx950 kernel runs, with
// the workgroup's threads stepped sequentially between barriers, so the index algebra, twiddle
// addressing, LDS padding and lazy ranges are checked on the CPU.  This is NOT a fallback path:
// it is not reachable from the C ABI and is only loaded by tests.
#define APSU_HOST_EMU 1
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "dev_consts.h"
#include "blake2x.h"
#include "bin_update.h"
#include "bin_lookup.h"
#include "bin_merge.h"
#include "bin_roots.h"
#include "bin_rows.h"
#include "bin_eval.h"
#include "bin_split.h"
#include "db_rebase.h"
#include "db_compact.h"
#include "db_place.h"
#include "multi_place.h"
#include "query_side.h"
#include "params.h"
#include "powers_dag.h"
#include "sched_policy.h"
#include "eval_plan.h"
#include "bundle_layout.h"
#include "mac_plan.h"
#include "cuckoo.h"

using namespace apsu_he;

// inverse transform whose first pass forms the dyadic tensor product while it loads (k_intt_tensor)
template <int LOGN, int MODE, int PASS, int C = 16, bool RAW = false> static void emu_pass_tensor(u64 *lds, u64 *glob, int T, const NttTable &tab, const SrcTensor &ops)
{
    if constexpr (PASS < plan_passes(LOGN, C)) {
        if constexpr (PASS == 0)           // as in ntt_body: products staged into the LDS image with coalesced loads
            for (int tid = 0; tid < T; tid++)
                for (int e = 2 * tid; e < (1 << LOGN); e += 2 * T) *reinterpret_cast<u64x2 *>(lds + lds_slot(e)) = src_load2(ops, glob, e, tab);
        for (int tid = 0; tid < T; tid++) {
            if constexpr (PASS == 0) ntt_pass<LOGN, true, MODE, 0, false, false, SrcTensor, true, TwInline, NoHook, C>(lds, glob, tid, T, tab, ops);   // (the source's input bound rides along, as in ntt_body)
            else ntt_pass<LOGN, true, MODE, PASS, 0, RAW, SrcPlain, false, TwInline, NoHook, C>(lds, glob, tid, T, tab);
        }
        emu_pass_tensor<LOGN, MODE, PASS + 1, C, RAW>(lds, glob, T, tab, ops);
    }
}

template <int LOGN, int C = 16> static void emu_intt_tensor(u64 *out, const NttTable &tab, int T, const SrcTensor &ops, bool raw = false)
{
    std::vector<u64> lds(lds_slots(1 << LOGN));
    if (raw) {                                                    // NTT_MAP_RAW: no twist, no closing reduction
        if (tab.narrow) emu_pass_tensor<LOGN, NTT_NARROW, 0, C, true>(lds.data(), out, T, tab, ops);
        else if (tab.wide_d4) emu_pass_tensor<LOGN, NTT_WIDE_NEAR, 0, C, true>(lds.data(), out, T, tab, ops);
        else emu_pass_tensor<LOGN, NTT_WIDE, 0, C, true>(lds.data(), out, T, tab, ops);
        return;
    }
    if (tab.narrow) emu_pass_tensor<LOGN, NTT_NARROW, 0, C>(lds.data(), out, T, tab, ops);
    else if (tab.wide_d4) emu_pass_tensor<LOGN, NTT_WIDE_NEAR, 0, C>(lds.data(), out, T, tab, ops);
    else emu_pass_tensor<LOGN, NTT_WIDE, 0, C>(lds.data(), out, T, tab, ops);
}

template <int LOGN, bool INV, int MODE, int PASS, int C = 16> static void emu_pass(u64 *lds, u64 *glob, int T, const NttTable &tab)
{
    if constexpr (PASS < plan_passes(LOGN, C)) {
        // in-place global reads/writes of a pass touch disjoint 16-coefficient sets per work item, so
        // stepping the threads sequentially is equivalent to the barrier-separated parallel execution
        if constexpr (INV && PASS == 0) {
            // as in k_ntt since round 5 (SrcStaged): the inverse stages its limb into the LDS image with coalesced loads and runs its first pass from there
            for (int tid = 0; tid < T; tid++)
                for (int e = 2 * tid; e < (1 << LOGN); e += 2 * T) *reinterpret_cast<u64x2 *>(lds + lds_slot(e)) = src_load2(SrcStaged(), glob, e, tab);
            for (int tid = 0; tid < T; tid++) ntt_pass<LOGN, true, MODE, 0, false, false, SrcPlain, true, TwInline, NoHook, C>(lds, glob, tid, T, tab);
        } else
            for (int tid = 0; tid < T; tid++) ntt_pass<LOGN, INV, MODE, PASS, 0, false, SrcPlain, false, TwInline, NoHook, C>(lds, glob, tid, T, tab);
        emu_pass<LOGN, INV, MODE, PASS + 1, C>(lds, glob, T, tab);
    }
}

template <int LOGN, bool INV, int MODE, int C = 16> static void emu_ntt_n(u64 *data, const NttTable &tab, int T)
{
    constexpr int N = 1 << LOGN;
    std::vector<u64> lds(lds_slots(N));
    emu_pass<LOGN, INV, MODE, 0, C>(lds.data(), data, T, tab);
    if (!INV) for (int e = 0; e < N; e++) data[e] = ntt_fwd_finish<MODE>(lds[lds_slot(e)], tab);
}

// C: coefficients per work item (16 = the throughput form, 8 = the latency form of round 6; ntt_core.h plan_k)
template <int LOGN, bool INV, int C = 16> static void emu_ntt(u64 *data, const NttTable &tab, int T)
{
    if (tab.narrow) emu_ntt_n<LOGN, INV, NTT_NARROW, C>(data, tab, T);
    else if (tab.wide_d4) emu_ntt_n<LOGN, INV, NTT_WIDE_NEAR, C>(data, tab, T);
    else emu_ntt_n<LOGN, INV, NTT_WIDE, C>(data, tab, T);
}

// One limb as k_ntt / k_ntt_gather run it, with the template arguments the kernels pass to ntt_body: RED 1 / 2 = forward transform of a limb
// gathered from `src` (reduced on load / taken as it is), RAW = the inverse leaves out its twist and its closing reduction
template <int LOGN, bool INV, int MODE, int PASS, int RED, bool RAW, int C> static void emu_pass_ex(u64 *lds, const u64 *src, u64 *glob, int T, const NttTable &tab)
{
    if constexpr (PASS < plan_passes(LOGN, C)) {
        if constexpr (PASS == 0 && RED != 0) {                    // forward only: pass 0 just reads, from the source limb
            for (int tid = 0; tid < T; tid++) ntt_pass<LOGN, INV, MODE, 0, RED, false, SrcPlain, false, TwInline, NoHook, C>(lds, const_cast<u64 *>(src), tid, T, tab);
        } else if constexpr (PASS == 0 && INV) {                  // SrcStaged: coalesced loads into the LDS image, the first pass from there
            for (int tid = 0; tid < T; tid++)
                for (int e = 2 * tid; e < (1 << LOGN); e += 2 * T) *reinterpret_cast<u64x2 *>(lds + lds_slot(e)) = src_load2(SrcStaged(), glob, e, tab);
            for (int tid = 0; tid < T; tid++) ntt_pass<LOGN, true, MODE, 0, 0, false, SrcStaged, true, TwInline, NoHook, C>(lds, glob, tid, T, tab, SrcStaged());
        } else if constexpr (PASS == 0) {
            for (int tid = 0; tid < T; tid++) ntt_pass<LOGN, INV, MODE, 0, 0, false, SrcPlain, false, TwInline, NoHook, C>(lds, glob, tid, T, tab);
        } else
            for (int tid = 0; tid < T; tid++) ntt_pass<LOGN, INV, MODE, PASS, 0, RAW, SrcPlain, false, TwInline, NoHook, C>(lds, glob, tid, T, tab);
        emu_pass_ex<LOGN, INV, MODE, PASS + 1, RED, RAW, C>(lds, src, glob, T, tab);
    }
}
template <int LOGN, bool INV, int MODE, int RED, bool RAW, int C> static void emu_ntt_ex_n(const u64 *src, u64 *data, const NttTable &tab, int T)
{
    constexpr int N = 1 << LOGN;
    std::vector<u64> lds(lds_slots(N));
    emu_pass_ex<LOGN, INV, MODE, 0, RED, RAW, C>(lds.data(), src, data, T, tab);
    if (!INV) for (int e = 0; e < N; e++) data[e] = ntt_fwd_finish<MODE>(lds[lds_slot(e)], tab);
}
template <int LOGN, int C> static void emu_ntt_ex(int inverse, int red, int raw, const u64 *src, u64 *data, const NttTable &tab, int T)
{
    // the kernels' wave-uniform branches: k_ntt (RED 0; RAW from the map entry), k_ntt_gather (RED 2 for a narrow modulus of a `nored` launch, else 1)
    if (inverse) {
        if (raw) {
            if (tab.narrow) emu_ntt_ex_n<LOGN, true, NTT_NARROW, 0, true, C>(src, data, tab, T);
            else if (tab.wide_d4) emu_ntt_ex_n<LOGN, true, NTT_WIDE_NEAR, 0, true, C>(src, data, tab, T);
            else emu_ntt_ex_n<LOGN, true, NTT_WIDE, 0, true, C>(src, data, tab, T);
        } else {
            if (tab.narrow) emu_ntt_ex_n<LOGN, true, NTT_NARROW, 0, false, C>(src, data, tab, T);
            else if (tab.wide_d4) emu_ntt_ex_n<LOGN, true, NTT_WIDE_NEAR, 0, false, C>(src, data, tab, T);
            else emu_ntt_ex_n<LOGN, true, NTT_WIDE, 0, false, C>(src, data, tab, T);
        }
    } else if (red == 0) {
        if (tab.narrow) emu_ntt_ex_n<LOGN, false, NTT_NARROW, 0, false, C>(src, data, tab, T);
        else if (tab.wide_d4) emu_ntt_ex_n<LOGN, false, NTT_WIDE_NEAR, 0, false, C>(src, data, tab, T);
        else emu_ntt_ex_n<LOGN, false, NTT_WIDE, 0, false, C>(src, data, tab, T);
    } else if (tab.narrow) {
        if (red == 2) emu_ntt_ex_n<LOGN, false, NTT_NARROW, 2, false, C>(src, data, tab, T);
        else emu_ntt_ex_n<LOGN, false, NTT_NARROW, 1, false, C>(src, data, tab, T);
    } else if (tab.wide_d4) emu_ntt_ex_n<LOGN, false, NTT_WIDE_NEAR, 1, false, C>(src, data, tab, T);
    else emu_ntt_ex_n<LOGN, false, NTT_WIDE, 1, false, C>(src, data, tab, T);
}

// forward transform whose load steps the bin's scaled coefficients to the next coset (k_bin_roots: SrcCoset through ntt_body's staged path)
template <int LOGN, int PASS> static void emu_pass_coset(u64 *lds, u64 *glob, int T, const NttTable &tab, const SrcCoset &ops)
{
    if constexpr (PASS < plan_passes(LOGN, 16)) {
        if constexpr (PASS == 0)
            for (int tid = 0; tid < T; tid++)
                for (int e = 2 * tid; e < (1 << LOGN); e += 2 * T) *reinterpret_cast<u64x2 *>(lds + lds_slot(e)) = src_load2(ops, glob, e, tab);
        for (int tid = 0; tid < T; tid++) {
            if constexpr (PASS == 0) ntt_pass<LOGN, false, NTT_NARROW, 0, 0, false, SrcCoset, true, TwInline, NoHook, 16>(lds, glob, tid, T, tab, ops);
            else ntt_pass<LOGN, false, NTT_NARROW, PASS, 0, false, SrcPlain, false, TwInline, NoHook, 16>(lds, glob, tid, T, tab);
        }
        emu_pass_coset<LOGN, PASS + 1>(lds, glob, T, tab, ops);
    }
}
template <int LOGN> static void emu_ntt_coset(u64 *row, const NttTable &tab, int T, const SrcCoset &ops)
{
    std::vector<u64> lds(lds_slots(1 << LOGN));
    emu_pass_coset<LOGN, 0>(lds.data(), row, T, tab, ops);
    for (int e = 0; e < (1 << LOGN); e++) row[e] = ntt_fwd_finish<NTT_NARROW>(lds[lds_slot(e)], tab);
}

// the product's transform tables for one modulus
struct EmuTables {
    std::vector<TwPair> fwd, dit, sc;
    NttTable tab;
    EmuTables(int logn, u64 q)
    {
        const size_t n = (size_t)1 << logn;
        const HeParams hp = HeParams::Create(n, { q }, 65537 < q ? 65537 : 3);
        const NttTablesHost &t = hp.ntt[0];
        fwd.resize(n); dit.resize(n); sc.resize(n);
        for (size_t k = 0; k < n; k++) {
            fwd[k] = { t.fwd[k], t.fwd_q[k] };
            dit[k] = { t.dit[k], t.dit_q[k] }; sc[k] = { t.scale[k], t.scale_q[k] };
        }
        tab = make_ntt_table(t, logn, fwd.data(), dit.data(), sc.data());
    }
};

static thread_local std::string g_err;

extern "C" {

const char *emu_last_error() { return g_err.c_str(); }

// NTT of one limb with the product's tables for modulus q (n = 2^logn); coeffs = coefficients per work item (16, or 8 where the ring
// size has the latency form: logn 12 and 13)
int emu_ntt_limb_c(int logn, int inverse, uint64_t q, uint64_t *data, int threads, int coeffs);
int emu_ntt_limb(int logn, int inverse, uint64_t q, uint64_t *data, int threads) { return emu_ntt_limb_c(logn, inverse, q, data, threads, 16); }
int emu_ntt_limb_c(int logn, int inverse, uint64_t q, uint64_t *data, int threads, int coeffs)
{
    try {
        if (coeffs != 16 && !(coeffs == 8 && plan_has_latency_form(logn))) throw std::invalid_argument("no pass schedule for this ring size and coefficients per work item");
        size_t n = (size_t)1 << logn;
        HeParams hp;   // only need tables: build for this single modulus via Create with K=1
        // plain modulus irrelevant for the tables; pick any value < q
        hp = HeParams::Create(n, { q }, 65537 < q ? 65537 : 3);
        const NttTablesHost &t = hp.ntt[0];
        std::vector<TwPair> fwd(n), dit(n), sc(n);
        for (size_t k = 0; k < n; k++) {
            fwd[k] = { t.fwd[k], t.fwd_q[k] };
            dit[k] = { t.dit[k], t.dit_q[k] }; sc[k] = { t.scale[k], t.scale_q[k] };
        }
        const NttTable tab = make_ntt_table(t, logn, fwd.data(), dit.data(), sc.data());
        if (coeffs == 8) {
            if (logn == 13) { if (inverse) emu_ntt<13, true, 8>(data, tab, threads); else emu_ntt<13, false, 8>(data, tab, threads); }
            else { if (inverse) emu_ntt<12, true, 8>(data, tab, threads); else emu_ntt<12, false, 8>(data, tab, threads); }
            return 0;
        }
#define CASE(L) case L: if (inverse) emu_ntt<L, true>(data, tab, threads); else emu_ntt<L, false>(data, tab, threads); break;
        switch (logn) { CASE(14) CASE(13) CASE(12) CASE(11) CASE(10) CASE(8) CASE(6) default: throw std::invalid_argument("unsupported logn"); }
#undef CASE
        return 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// The same with the kernels' other template arguments (tests/test_ntt_step_model_cpu.py): red 0 = in place on data; 1 / 2 = the forward
// transform of `src` (another modulus' residues reduced on load / any words taken as they are: k_ntt_gather with nored 0 / 1) written to
// data; raw = the inverse transform without its twist and closing reduction (NTT_MAP_RAW).  Refused: red with an inverse transform or
// without a source, raw with a forward one, red 2 for a modulus that is not narrow (the kernel reduces there).
int emu_ntt_limb_ex(int logn, int inverse, uint64_t q, const uint64_t *src, uint64_t *data, int threads, int coeffs, int red, int raw)
{
    try {
        if (coeffs != 16 && !(coeffs == 8 && plan_has_latency_form(logn))) throw std::invalid_argument("no pass schedule for this ring size and coefficients per work item");
        if (red < 0 || red > 2 || (red && (inverse || !src)) || (raw && !inverse)) throw std::invalid_argument("red is for a forward transform with a source, raw for an inverse one");
        const EmuTables et(logn, q);
        if (red == 2 && !et.tab.narrow) throw std::invalid_argument("an unreduced gather needs a narrow modulus");
        if (coeffs == 8) {
            if (logn == 13) emu_ntt_ex<13, 8>(inverse, red, raw, src, data, et.tab, threads); else emu_ntt_ex<12, 8>(inverse, red, raw, src, data, et.tab, threads);
            return 0;
        }
#define CASE(L) case L: emu_ntt_ex<L, 16>(inverse, red, raw, src, data, et.tab, threads); break;
        switch (logn) { CASE(14) CASE(13) CASE(12) CASE(11) CASE(10) CASE(8) CASE(6) default: throw std::invalid_argument("unsupported logn"); }
#undef CASE
        return 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}
// ntt_reduce128_lazy on explicit (hi, lo) pairs, then ntt_lazy_bound_q and ntt_lazy_input_ok(logn) in out[count], out[count + 1];
// returns fold_k, 0 when the modulus does not admit the fold
int emu_reduce128_lazy(uint64_t q, int logn, const uint64_t *hi, const uint64_t *lo, uint64_t *out, int count)
{
    const NttTable tab = make_ntt_table(q, logn);
    if (!ntt_fold128_ok(tab.fold_k, tab.fold_c)) return 0;
    for (int i = 0; i < count; i++) out[i] = ntt_reduce128_lazy(hi[i], lo[i], tab);
    out[count] = ntt_lazy_bound_q(tab);
    out[count + 1] = plan_passes(logn, 16) ? (u64)ntt_lazy_input_ok(tab, logn) : 0;
    return (int)tab.fold_k;
}

// INTT(x0*y0 (+ x1*y1)) of one limb through the fused loader; x1 = y1 = NULL for a single product.  Returns -2 when the
// modulus does not admit the 128-bit fold reduction (the engine then keeps the separate tensor kernel).
int emu_intt_tensor_limb_c(int logn, uint64_t q, const uint64_t *x0, const uint64_t *y0, const uint64_t *x1, const uint64_t *y1,
                           uint64_t *out, int threads, int coeffs);
int emu_intt_tensor_limb(int logn, uint64_t q, const uint64_t *x0, const uint64_t *y0, const uint64_t *x1, const uint64_t *y1,
                         uint64_t *out, int threads)
{
    return emu_intt_tensor_limb_c(logn, q, x0, y0, x1, y1, out, threads, 16);
}
int emu_intt_tensor_limb_c(int logn, uint64_t q, const uint64_t *x0, const uint64_t *y0, const uint64_t *x1, const uint64_t *y1,
                           uint64_t *out, int threads, int coeffs)
{
    try {
        if ((coeffs & 0xff) != 16 && !((coeffs & 0xff) == 8 && plan_has_latency_form(logn))) throw std::invalid_argument("no pass schedule for this ring size and coefficients per work item");
        size_t n = (size_t)1 << logn;
        HeParams hp = HeParams::Create(n, { q }, 65537 < q ? 65537 : 3);
        const NttTablesHost &t = hp.ntt[0];
        std::vector<TwPair> fwd(n), dit(n), sc(n);
        for (size_t k = 0; k < n; k++) {
            fwd[k] = { t.fwd[k], t.fwd_q[k] };
            dit[k] = { t.dit[k], t.dit_q[k] }; sc[k] = { t.scale[k], t.scale_q[k] };
        }
        const NttTable tab = make_ntt_table(t, logn, fwd.data(), dit.data(), sc.data());
        if (!ntt_fold128_ok(tab.fold_k, tab.fold_c)) return -2;
        // coeffs | 0x100: the products enter as the fold's last word (< 4q) where the engine would take them so (k_intt_tensor: ntt_lazy_input_ok)
        // coeffs | 0x200: the limb's map entry carries NTT_MAP_RAW
        const bool lazy = (coeffs & 0x100) != 0, raw = (coeffs & 0x200) != 0;
        coeffs &= 0xff;
        if (lazy && !ntt_lazy_input_ok(tab, logn)) return -3;
        const SrcTensor ops{ x0, y0, x1, y1, lazy };
        if (coeffs == 8) {
            if (logn == 13) emu_intt_tensor<13, 8>(out, tab, threads, ops, raw); else emu_intt_tensor<12, 8>(out, tab, threads, ops, raw);
            return 0;
        }
#define CASE(L) case L: emu_intt_tensor<L>(out, tab, threads, ops, raw); break;
        switch (logn) { CASE(14) CASE(13) CASE(12) CASE(11) CASE(10) CASE(8) CASE(6) default: throw std::invalid_argument("unsupported logn"); }
#undef CASE
        return 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// `count` 32-bit outputs of the Blake2xb generator (blake2x.h, the code k_fill_blake2xb runs) starting at output `first`
int emu_blake2xb_values(const uint64_t *seed, uint64_t first, uint32_t *out, int count)
{
    Blake2xbSeed sd;
    for (int i = 0; i < 8; i++) sd.w[i] = seed[i];
    u64 blk[8];
    u64 have = ~(u64)0;
    for (int i = 0; i < count; i++) {
        const u64 g = first + (u64)i;
        if (g / 16 != have) { have = g / 16; blake2xb_stream_block(sd, have, blk); }
        out[i] = blake2xb_stream_u32(blk, (unsigned)(g % 16));
    }
    return 0;
}

// N5 (query_side.h, the functions k_sample_ternary / k_sample_cbd / k_plain_powers run): the secret's n coefficients under `seed`
int emu_qs_secret(const uint64_t *seed, uint64_t n, int8_t *out)
{
    Blake2xbSeed sd;
    for (int i = 0; i < 8; i++) sd.w[i] = seed[i];
    u64 blk[8];
    for (u64 k = 0; k < n; k++) {
        if (k % 8 == 0) blake2xb_stream_block(sd, qs_secret_block(k), blk);
        out[k] = (int8_t)qs_ternary(blk[k % 8]);
    }
    return 0;
}
// the noise polynomial of `object`
int emu_qs_noise(const uint64_t *seed, uint64_t object, uint64_t n, int8_t *out)
{
    Blake2xbSeed sd;
    for (int i = 0; i < 8; i++) sd.w[i] = seed[i];
    u64 blk[8];
    for (u64 k = 0; k < n; k++) {
        if (k % 8 == 0) blake2xb_stream_block(sd, qs_noise_block(object, k), blk);
        out[k] = (int8_t)qs_cbd(blk[k % 8]);
    }
    return 0;
}
// the public seed of `object` (eight words)
int emu_qs_public_seed(const uint64_t *seed, uint64_t object, uint64_t *out)
{
    Blake2xbSeed sd;
    for (int i = 0; i < 8; i++) sd.w[i] = seed[i];
    blake2xb_stream_block(sd, qs_seed_block(object), out);
    return 0;
}
// the layout's constants: max n, blocks per polynomial, key objects, max objects, first block of the secret / seed / noise ranges
int emu_qs_layout(uint64_t *out, int cap)
{
    const u64 v[7] = { QS_MAX_N, QS_POLY_BLOCKS, QS_KEY_OBJECTS, QS_MAX_OBJECTS, QS_SECRET_BLOCK0, QS_SEED_BLOCK0, QS_NOISE_BLOCK0 };
    for (int i = 0; i < 7 && i < cap; i++) out[i] = v[i];
    return 7;
}
// first stream block of coefficient k's draw: kind 0 secret, 1 public seed of `object`, 2 noise of `object`
uint64_t emu_qs_block(int kind, uint64_t object, uint64_t k)
{
    return kind == 0 ? qs_secret_block(k) : kind == 1 ? qs_seed_block(object) : qs_noise_block(object, k);
}
int emu_qs_pow_mod(uint64_t t, const uint64_t *x, const uint32_t *e, uint64_t *out, int count)
{
    ModulusInfo mi(t);
    const Mod m{ t, mi.ratio[0], mi.ratio[1] };
    for (int i = 0; i < count; i++) out[i] = qs_pow_mod(x[i], e[i], m);
    return 0;
}

// ntt_reduce128_fold on explicit (hi, lo) pairs; returns 0 when the modulus does not admit it
int emu_reduce128(uint64_t q, const uint64_t *hi, const uint64_t *lo, uint64_t *out, int count)
{
    const NttTable tab = make_ntt_table(q, 0);                  // (the reductions do not look at the transform's depth)
    if (!ntt_fold128_ok(tab.fold_k, tab.fold_c)) return 0;
    for (int i = 0; i < count; i++) out[i] = ntt_reduce128_fold(hi[i], lo[i], tab);
    return (int)tab.fold_k;
}

// ntt_reduce_any (the fold / Barrett final reduction of the NTT kernels) on explicit values; returns fold_k
int emu_reduce_any(uint64_t q, const uint64_t *x, uint64_t *out, int count)
{
    const NttTable tab = make_ntt_table(q, 0);
    for (int i = 0; i < count; i++) out[i] = ntt_reduce_any(x[i], tab);
    return (int)tab.fold_k;
}

// The scheduler's ordering rules (sched_policy.h), for exhaustive enumeration by tests/test_host_logic.py.
// bits: 0 recycled, 1 last_use_set, 2 last_use_done, 3 high_async, 4 split_ok, 5 prof_on, 6 pipe_cp, 7 force_pipe, 8 inputs_ready,
// 9 on_device, 10 device_busy.  Returns walk | main_waits_high_ready << 2 | side_waits_last_use << 3 | side_waits_main << 4 | consumes_last_use << 5.
int emu_plan_walk(unsigned bits, int split_mode)
{
    WalkState s{};
    s.recycled = bits & 1; s.last_use_set = bits & 2; s.last_use_done = bits & 4; s.high_async = bits & 8; s.split_ok = bits & 16;
    s.prof_on = bits & 32; s.pipe_cp = bits & 64; s.force_pipe = bits & 128; s.inputs_ready = bits & 256; s.on_device = bits & 512;
    s.device_busy = bits & 1024; s.split_mode = split_mode;
    const WalkPlan p = plan_walk(s);
    return p.walk | (p.main_waits_high_ready ? 4 : 0) | (p.side_waits_last_use ? 8 : 0) | (p.side_waits_main ? 16 : 0) | (p.consumes_last_use ? 32 : 0);
}
// entry i: bit 0 fits, bit 1 last_use_set, bit 2 last_use_done
int emu_pick_pooled_buffer(const unsigned char *entries, int count, int inputs_ready)
{
    std::vector<PoolEntryState> st(count);
    for (int i = 0; i < count; i++) st[i] = PoolEntryState{ (entries[i] & 1) != 0, (entries[i] & 2) != 0, (entries[i] & 4) != 0 };
    return pick_pooled_buffer(st.data(), st.size(), inputs_ready != 0);
}

// The form decisions of the Paterson-Stockmeyer evaluation (eval_plan.h), for enumeration by tests/test_host_logic.py.
// bits: 0 high_in_flight, 1 eval_side, 2 prof_on, 3 force_per_term, 4 fuse_tensor, 5 fuse_tail, 6 lane2, 7 on_lane0.  Returns i0_fast |
// need_vlast << 1 | raw_drop << 2 | raw_i0 << 3 | fused_drop << 4 | summed << 5 | side << 6 | side_i0 << 7 | wait_high_ready << 8 |
// fuse_tensor << 9 | fuse_tail << 10 | cf << 11 | i0 << 13.
int emu_plan_eval(unsigned bits, int low, int high, int L, int nB, uint32_t l, uint64_t q_last, uint64_t q_widest, int Bs, int max_terms)
{
    EvalState s{};
    s.low = low; s.high = high; s.L = L; s.nB = nB; s.l = l; s.q_last = q_last; s.q_widest = q_widest; s.Bs = Bs; s.max_terms = max_terms;
    s.high_in_flight = bits & 1; s.eval_side = bits & 2; s.prof_on = bits & 4; s.force_per_term = bits & 8; s.fuse_tensor = bits & 16;
    s.fuse_tail = bits & 32; s.lane2 = bits & 64; s.on_lane0 = bits & 128;
    const EvalPlan p = plan_eval(s);
    return (int)p.i0_fast | p.need_vlast << 1 | p.raw_drop << 2 | p.raw_i0 << 3 | p.fused_drop << 4 | p.summed << 5 | p.side << 6 | p.side_i0 << 7 |
           p.wait_high_ready << 8 | p.fuse_tensor << 9 | p.fuse_tail << 10 | p.cf << 11 | p.i0 << 13;
}
int emu_behz_unrolled(int L, int nB) { return behz_unrolled(L, nB); }

// The stored layout of a BinBundle (bundle_layout.h), for enumeration by tests/test_bundle_layout_cpu.py.  out = use_ps, H, r, pt_level,
// ntt_count, lifted_count, the number of runs, then d0, count, kind, first_slot per run; where (may be null): kind, slot of
// d = 0 .. degree.  Returns the words of `out` (the first `cap` are written), or -1 for a refused shape (emu_last_error).
int emu_bundle_layout(uint32_t ps_low_degree, uint32_t degree, int first_chain_idx, uint64_t *out, int cap, uint32_t *where)
{
    try {
        const BundleLayout y = bundle_layout(ps_low_degree, degree, first_chain_idx);
        std::vector<u64> v{ y.use_ps, y.H, y.r, (u64)y.pt_level, y.ntt_count, y.lifted_count, y.runs.size() };
        for (const BundleRun &r : y.runs) v.insert(v.end(), { r.d0, r.count, (u64)r.kind, r.first_slot });
        for (size_t i = 0; i < v.size() && (int)i < cap; i++) out[i] = v[i];
        for (uint32_t d = 0; where && d <= degree; d++) { where[2 * d] = (uint32_t)y.where(d).kind; where[2 * d + 1] = y.where(d).slot; }
        return (int)v.size();
    } catch (const std::invalid_argument &e) { g_err = e.what(); return -1; }
}

// The launch form of the transform (ntt_form.h), for tabulation by tests/test_host_logic.py: out = threads, coeffs_per_lane, min_waves, split
void emu_ntt_form(int logn, int kind, size_t limbs, size_t latency_limbs, int narrow, int *out)
{
    const NttForm f = ntt_form(logn, (NttKind)kind, limbs, latency_limbs, narrow != 0);
    out[0] = f.threads; out[1] = f.coeffs_per_lane; out[2] = f.min_waves; out[3] = f.split;
}

// PSUParams::Load + HeParams: returns derived numbers for comparison with the oracle
int emu_params_info(const char *json, uint64_t *out, int cap)
{
    try {
        PSUParams p = PSUParams::Load(json);
        HeParams hp = HeParams::FromPSUParams(p);
        std::vector<u64> v;
        v.push_back(hp.n); v.push_back(hp.K); v.push_back(hp.first_chain_idx); v.push_back(hp.t);
        for (u64 q : hp.key_q) v.push_back(q);
        for (int j = 0; j < hp.K; j++) v.push_back(hp.ntt[j].psi);
        const LevelConstants &lv = hp.level[hp.first_chain_idx];
        v.push_back(lv.nB); v.push_back(lv.m_sk); v.push_back(lv.gamma);
        for (u64 b : lv.B) v.push_back(b);
        v.push_back(p.bundle_idx_count); v.push_back(p.items_per_bundle); v.push_back(p.item_bit_count);
        v.push_back(hp.irrelevant_bit_count);
        for (size_t i = 0; i < v.size() && (int)i < cap; i++) out[i] = v[i];
        return (int)v.size();
    } catch (const std::invalid_argument &e) { g_err = e.what(); return -1;
    } catch (const std::exception &e) { g_err = e.what(); return -2; }
}

// The auxiliary BEHZ base HeParams picks for a parameter file (narrow = 1: AuxBase::Narrow, the engine's default; 0: SEAL's).
// out = aux_narrow, aux_bits, logn, levels, then per level L, nB, m_sk, gamma, B_0 .. B_{nB-1}.  aux_note (why SEAL's base was kept)
// is left in emu_last_error.
int emu_aux_base(const char *json, int narrow, uint64_t *out, int cap)
{
    try {
        PSUParams p = PSUParams::Load(json);
        HeParams hp = HeParams::FromPSUParams(p, narrow ? AuxBase::Narrow : AuxBase::Seal);
        std::vector<u64> v;
        v.push_back(hp.aux_narrow); v.push_back((u64)hp.aux_bits); v.push_back((u64)hp.logn); v.push_back(hp.level.size());
        for (const LevelConstants &lv : hp.level) {
            v.push_back(lv.L); v.push_back(lv.nB); v.push_back(lv.m_sk); v.push_back(lv.gamma);
            for (u64 b : lv.B) v.push_back(b);
        }
        g_err = hp.aux_note;
        for (size_t i = 0; i < v.size() && (int)i < cap; i++) out[i] = v[i];
        return (int)v.size();
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// The constant blocks a context uploads (dev_consts.h: build_device_constants), for tests/test_dev_consts_cpu.py.  The context comes
// from a parameter file (json) or, with json = NULL, from HeParams::Create(n, primes[k], t); narrow = 1: AuxBase::Narrow, the engine's
// default, 0: SEAL's base.  block: tw, tabs, fin, drop, levels, map_ext, map_ext_fin, map_ks, map_ksacc, map_ksacc_raw, map_ct, mdtw, key,
// key_level, max_multiple (u64 per key prime), scalars (u64: data_primes_narrow, ext_primes_narrow, unlift_exact, then
// packed_row_bits per key prime).  A block is the bytes the engine uploads (arrays of TwPair / NttTable / ShoupConst / DevLevel / int,
// one DevKey; padding is zero), except that every pointer member holds its table reference: 1 + the element offset into the table it
// points into (16-byte elements), 0 for null.  Returns the block's size in bytes (copied to out when cap is large enough), or -1.
int64_t emu_device_constants(const char *json, uint64_t n, const uint64_t *primes, int k, uint64_t t, int narrow, const char *block, void *out,
                             uint64_t cap)
{
    try {
        const AuxBase aux = narrow ? AuxBase::Narrow : AuxBase::Seal;
        const HeParams hp = json ? HeParams::FromPSUParams(PSUParams::Load(json), aux) : HeParams::Create((size_t)n, std::vector<u64>(primes, primes + k), t, aux);
        const DeviceConstants dc = build_device_constants(hp);
        std::vector<u64> scalars{ dc.data_primes_narrow, dc.ext_primes_narrow, dc.unlift_exact };
        scalars.insert(scalars.end(), dc.row_bits.begin(), dc.row_bits.end());
        const std::string b = block;
        const void *p = nullptr;
        size_t bytes = 0;
        auto take = [&](const char *name, const auto &v) { if (b == name) { p = v.data(); bytes = v.size() * sizeof(v[0]); } return b == name; };
        if (b == "key") { p = &dc.key; bytes = sizeof(DevKey); }
        else if (!(take("tw", dc.tw) || take("tabs", dc.tabs) || take("fin", dc.fin) || take("drop", dc.drop) || take("levels", dc.levels) ||
                   take("map_ext", dc.map_ext) || take("map_ext_fin", dc.map_ext_fin) || take("map_ks", dc.map_ks) || take("map_ksacc", dc.map_ksacc) ||
                   take("map_ksacc_raw", dc.map_ksacc_raw) || take("map_ct", dc.map_ct) || take("mdtw", dc.mdtw) || take("key_level", dc.key_level) ||
                   take("max_multiple", dc.max_multiple) || take("scalars", scalars)))
            throw std::invalid_argument("unknown block");
        if (bytes && bytes <= cap) std::memcpy(out, p, bytes);
        return (int64_t)bytes;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}
// sizeof NttTable, DevLevel, DevKey, then DMAXL, DMAXB (the test's mirror of the layouts checks itself against these)
void emu_dev_layout(uint64_t *out) { out[0] = sizeof(NttTable); out[1] = sizeof(DevLevel); out[2] = sizeof(DevKey); out[3] = DMAXL; out[4] = DMAXB; }

// make_ntt_table for modulus q and `logn` stages: out = q, ninv, ninv_q, r1, r0, narrow, fold_k, fold_c, wide_d4.  with_tables = 1: the
// form that takes the modulus' tables (q = 1 mod 2^(logn+1)); 0: the modulus-only form (ninv = ninv_q = 0)
int emu_ntt_table(uint64_t q, int logn, int with_tables, uint64_t *out)
{
    try {
        const NttTable tab = with_tables ? make_ntt_table(HeParams::Create((size_t)1 << logn, { q }, 65537 < q ? 65537 : 3).ntt[0], logn, nullptr, nullptr, nullptr)
                                         : make_ntt_table(q, logn);
        const u64 v[9] = { tab.q, tab.ninv, tab.ninv_q, tab.r1, tab.r0, (u64)tab.narrow, tab.fold_k, tab.fold_c, tab.wide_d4 };
        for (int i = 0; i < 9; i++) out[i] = v[i];
        return 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// read_switches() under the caller's environment: two_stream_default, eval_side, packed_rows, eval_ws_bytes, arena_bytes, force_per_term,
// mac_kara, seed_expand_host, fuse_tail, ntt_latency_limbs (signed values as int64)
void emu_switches(int64_t *out)
{
    const EngineSwitches s = read_switches();
    const int64_t v[10] = { s.two_stream_default, s.eval_side, s.packed_rows, (int64_t)s.eval_ws_bytes, (int64_t)s.arena_bytes, s.force_per_term,
                            s.mac_kara, s.seed_expand_host, s.fuse_tail, (int64_t)s.ntt_latency_limbs };
    for (int i = 0; i < 10; i++) out[i] = v[i];
}

// PowersDag::configure on explicit sets; nodes: [power, depth, p1, p2] ascending by power
int emu_powers_dag(const uint32_t *sources, int ns, const uint32_t *targets, int nt, uint32_t *nodes)
{
    PowersDag d;
    if (!d.configure(std::set<uint32_t>(sources, sources + ns), std::set<uint32_t>(targets, targets + nt))) return -1;
    int i = 0;
    for (auto &kv : d.nodes()) {
        nodes[4 * i + 0] = kv.second.power; nodes[4 * i + 1] = kv.second.depth;
        nodes[4 * i + 2] = kv.second.parents.first; nodes[4 * i + 3] = kv.second.parents.second;
        i++;
    }
    return (int)d.depth();
}

int emu_create_powers_set(uint32_t ps_low, uint32_t target, uint32_t *out, int cap)
{
    try {
        auto s = create_powers_set(ps_low, target);
        int i = 0;
        for (uint32_t p : s) { if (i < cap) out[i] = p; i++; }
        return i;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// level constants flattened for diffing against the oracle (test_constants)
int emu_level_constants(uint64_t n, const uint64_t *q, int k, uint64_t t, int chain_idx, uint64_t *out, int cap)
{
    try {
        HeParams hp = HeParams::Create((size_t)n, std::vector<u64>(q, q + k), t);
        const LevelConstants &lv = hp.level.at(chain_idx);
        std::vector<u64> v;
        auto put = [&](const std::vector<u64> &a) { for (u64 x : a) v.push_back(x); };
        v.push_back(lv.L); v.push_back(lv.nB); v.push_back(lv.m_sk); v.push_back(lv.gamma);
        put(lv.B); put(lv.coeff_div_plain); v.push_back(lv.q_mod_t); v.push_back(lv.upper_half_threshold);
        put(lv.upper_half_incr); put(lv.inv_q_last); put(lv.inv_punct_q);
        for (auto &r : lv.q_to_bsk) put(r);
        put(lv.q_to_mtilde); v.push_back(lv.neg_inv_q_mod_mtilde);
        put(lv.prod_q_mod_bsk); put(lv.inv_prod_q_mod_bsk); put(lv.inv_mtilde_mod_bsk); put(lv.inv_punct_B);
        for (auto &r : lv.B_to_q) put(r);
        put(lv.B_to_msk); v.push_back(lv.inv_prod_B_mod_msk); put(lv.prod_B_mod_q); put(hp.inv_p_mod_q);
        for (size_t i = 0; i < v.size() && (int)i < cap; i++) out[i] = v[i];
        return (int)v.size();
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// k_bins_update on one bin, as the wave runs it (bin_update.h): coefficient i in lane i % 64, register slot i / 64, every shuffle an
// explicit loop over the 64 lanes.  in / out: `rows` coefficients mod t (out may alias nothing; it is written on success only).
// Removals first, then insertions.  Returns the new count (index of the highest non-zero coefficient) or -1 with
// status[0] = 1: rem[status[1]] left a remainder; 2: the zero polynomial (not a bin); 3: the result needs more than `rows` coefficients.
int64_t emu_bin_update(uint64_t t_, const uint64_t *in, uint32_t rows, const uint64_t *rem, uint32_t n_rem, const uint64_t *ins, uint32_t n_ins,
                       uint64_t *out, int64_t *status)
{
    const ModulusInfo mi(t_);
    const Mod t{ t_, mi.ratio[0], mi.ratio[1] };
    constexpr int W = BIN_LANES;
    const int slots = (int)((rows + W - 1) / W);
    std::vector<std::vector<u64>> P(slots, std::vector<u64>(W, 0));
    int top = -1;
    for (int j = 0; j < slots; j++)
        for (int lane = 0; lane < W; lane++) {
            const u32 d = (u32)(j * W + lane);
            P[j][lane] = d < rows ? in[d] : 0;
            if (P[j][lane]) top = std::max(top, (int)d);          // the wave's max-reduction
        }
    status[0] = status[1] = 0;
    if (top < 0) { status[0] = 2; return -1; }
    u32 cnt = (u32)top;
    for (u32 r = 0; r < n_rem; r++) {
        const u64 a = rem[r];
        const int jmax = (int)(cnt >> 6);
        u64 carry = 0;
        for (int j = slots - 1; j >= 0; j--) {
            if (j > jmax) continue;
            std::vector<ScanPair> p(W);
            for (int lane = 0; lane < W; lane++) p[lane] = ScanPair{ a, P[j][lane] };
            for (int o = 1; o < W; o <<= 1) {
                std::vector<ScanPair> up(W);
                for (int lane = 0; lane < W; lane++) up[lane] = p[lane + o < W ? lane + o : lane];      // __shfl_down
                for (int lane = 0; lane < W; lane++) if (lane + o < W) p[lane] = bin_scan_compose(p[lane], up[lane], t);
            }
            std::vector<u64> sv(W);
            for (int lane = 0; lane < W; lane++) sv[lane] = bin_scan_carry(p[lane], carry, t);
            for (int lane = 0; lane < W; lane++) P[j][lane] = lane == W - 1 ? carry : sv[lane + 1];
            carry = sv[0];
        }
        if (carry != 0) { status[0] = 1; status[1] = r; return -1; }
        cnt--;
    }
    for (u32 r = 0; r < n_ins; r++) {
        if (cnt + 2 > rows) { status[0] = 3; return -1; }
        const u64 a = ins[r], neg_a = a ? t.q - a : 0;
        const int jmax = (int)((cnt + 1) >> 6);
        for (int j = slots - 1; j >= 0; j--) {
            if (j > jmax) continue;
            std::vector<u64> prev(W);
            for (int lane = 0; lane < W; lane++) prev[lane] = lane ? P[j][lane - 1] : (j > 0 ? P[j - 1][W - 1] : 0);
            for (int lane = 0; lane < W; lane++) P[j][lane] = bin_insert_step(P[j][lane], prev[lane], neg_a, t);
        }
        cnt++;
    }
    for (u32 d = 0; d < rows; d++) out[d] = P[d / W][d % W];
    return (int64_t)cnt;
}

uint64_t emu_bin_unlift(uint64_t x, uint64_t t, uint64_t q0) { return bin_unlift(x, t, q0); }

// k_bin_counts over poly[rows][n]: one lane per slot, rows walked from the top
void emu_bin_counts(const uint64_t *poly, uint64_t n, uint32_t rows, uint32_t *counts)
{
    for (size_t i = 0; i < n; i++) {
        int top = (int)rows - 1;
        while (top >= 0 && poly[(size_t)top * n + i] == 0) top--;
        counts[i] = bin_count_of(top);
    }
}

// k_bins_lookup<R> over poly[degree + 1][n] as the waves run it (bin_lookup.h): the points laid out by lookup_plan, one wave per work
// item, an explicit loop over its 64 lanes, R accumulators per lane, rows from the top four at a time.  flags[count * F] must come in
// as 0xEE: a part that no lane writes keeps it.  stats (may be null): work items, rows of point storage, largest nrows of a work item.
// Returns 0, or -1 (emu_last_error) for an entry that does not lie inside the n slots or an R outside 1 .. 16.
int emu_bins_lookup(uint64_t t_, const uint64_t *poly, uint64_t n, uint32_t degree, const uint64_t *felts, const uint32_t *start, uint64_t count,
                    uint32_t F, int R, unsigned char *flags, uint64_t *stats)
{
    try {
        if (R < 1 || R > 16) throw std::invalid_argument("R out of range");
        for (size_t e = 0; e < count; e++)
            if ((u64)start[e] + F > n) throw std::invalid_argument("entry beyond the last slot");
        const ModulusInfo mi(t_);
        const Mod t{ t_, mi.ratio[0], mi.ratio[1] };
        const LookupPlan plan = lookup_plan(felts, start, count, F, n, R);
        u32 widest = 0;
        for (const LookupWork &wk : plan.work) {
            widest = std::max(widest, wk.nrows);
            for (u32 lane = 0; lane < LOOKUP_LANES; lane++) {
                const size_t slot = (size_t)wk.tile * LOOKUP_LANES + lane;
                const bool live = slot < n;
                const u64 *col = poly + (live ? slot : 0);
                u64 x[16], acc[16];
                for (int r = 0; r < R; r++) {
                    x[r] = (u32)r < wk.nrows ? plan.pts[((size_t)wk.row0 + r) * LOOKUP_LANES + lane] : 0;
                    acc[r] = 0;
                }
                u64 nz = 0;
                int d = (int)degree;
                for (; d >= 3; d -= 4) {
                    u64 p[4];
                    for (int k = 0; k < 4; k++) p[k] = col[(size_t)(d - k) * n];
                    for (int k = 0; k < 4; k++) {
                        nz |= p[k];
                        for (int r = 0; r < R; r++) acc[r] = lookup_horner_step(acc[r], x[r], p[k], t);
                    }
                }
                for (; d >= 0; d--) {
                    const u64 p = col[(size_t)d * n];
                    nz |= p;
                    for (int r = 0; r < R; r++) acc[r] = lookup_horner_step(acc[r], x[r], p, t);
                }
                for (int r = 0; r < R && (u32)r < wk.nrows; r++) {
                    const u32 part = plan.idx[((size_t)wk.row0 + r) * LOOKUP_LANES + lane];
                    if (part != LOOKUP_NONE) flags[part] = live && lookup_found(acc[r], nz) ? 1 : 0;
                }
            }
        }
        if (stats) { stats[0] = plan.work.size(); stats[1] = plan.rows(); stats[2] = widest; }
        return 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// k_bins_eval over poly[rows][n] as the waves run it (bin_eval.h): one wave per tile of 64 slots, the tile's top from the counts of
// emu_bin_counts, an explicit loop over its 64 lanes, rows from the top EVAL_ROWS at a time.  mask, is_bin and walked may be null;
// out[n] and is_bin[n] must come in as 0xEE bytes (a word that no lane writes keeps them); walked[tiles] = the rows a tile read.
// wide: 0 = the width the launch takes for t, 1 = the 128-bit step whatever t (both must agree wherever both are exact).
// Returns 0, or -1 (emu_last_error) for a value that is not below t.
int emu_bins_eval(uint64_t t_, const uint64_t *poly, uint64_t n, uint32_t rows, const uint64_t *x, const uint64_t *mask, int wide, uint64_t *out,
                  unsigned char *is_bin, uint32_t *walked)
{
    try {
        for (size_t s = 0; s < n; s++)
            if (x[s] >= t_ || (mask && mask[s] >= t_)) throw std::invalid_argument("slot value is not reduced modulo the plain modulus");
        const ModulusInfo mi(t_);
        const Mod t{ t_, mi.ratio[0], mi.ratio[1] };
        const bool narrow = !wide && merge_narrow(merge_bits(t_));
        std::vector<u32> counts(n);
        emu_bin_counts(poly, n, rows, counts.data());
        const size_t tiles = (n + EVAL_LANES - 1) / EVAL_LANES;
        for (size_t tile = 0; tile < tiles; tile++) {
            int top = -1;
            for (int lane = 0; lane < EVAL_LANES; lane++) {
                const size_t slot = tile * EVAL_LANES + lane;
                top = std::max(top, eval_count_top(slot < n ? counts[slot] : LOOKUP_NONE));
            }
            const int d0 = eval_walk_top(top, rows);
            if (walked) walked[tile] = (uint32_t)(d0 + 1);
            for (int lane = 0; lane < EVAL_LANES; lane++) {
                const size_t slot = tile * EVAL_LANES + lane;
                if (slot >= n) continue;
                const u64 *col = poly + slot;
                const u64 xs = x[slot];
                const u64 acc = narrow ? eval_walk<true>(col, n, d0, xs, t) : eval_walk<false>(col, n, d0, xs, t);
                out[slot] = eval_finish(acc, mask ? mask[slot] : 0, t);
                if (is_bin) is_bin[slot] = eval_is_bin(counts[slot]) ? 1 : 0;
            }
        }
        return 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}
int emu_eval_rows() { return EVAL_ROWS; }

// self_test_reduce over `count` reports (bin_eval.h), each sizeof(SelfTestReport) bytes; emu_self_test_report_bytes gives the size
int emu_self_test_report_bytes() { return (int)sizeof(SelfTestReport); }
void emu_self_test_reduce(const void *parts, int count, void *out)
{
    SelfTestReport r = self_test_empty();
    for (int i = 0; i < count; i++) self_test_reduce(r, static_cast<const SelfTestReport *>(parts)[i]);
    *static_cast<SelfTestReport *>(out) = r;
}

// ---- reading the bins back (bin_roots.h)
uint64_t emu_field_generator(uint64_t t)
{
    try { return field_generator(t); } catch (const std::exception &e) { g_err = e.what(); return 0; }
}

// (t - 1) / n, or -1 with emu_last_error for a modulus the walk cannot serve
int64_t emu_roots_coset_count(uint64_t t, uint64_t n)
{
    try { return (int64_t)roots_coset_count(t, n); } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

int emu_ntt_limb_c(int logn, int inverse, uint64_t q, uint64_t *data, int threads, int coeffs);
// the point table: the forward transform mod t of the polynomial X, through the library transform's emulation
int emu_roots_points(int logn, uint64_t t, uint64_t *pts)
{
    const size_t n = (size_t)1 << logn;
    std::fill(pts, pts + n, 0);
    pts[1] = 1;
    return emu_ntt_limb_c(logn, 0, t, pts, (int)std::max<size_t>(64, n / 16), 16);
}

// the coset walk alone: out[j * n + k] = c_j pts[k], the evaluation point of output position k of coset j, j < (t - 1) / n
int emu_roots_walk(int logn, uint64_t t, uint64_t *out)
{
    try {
        const size_t n = (size_t)1 << logn;
        const u32 cosets = roots_coset_count(t, n);
        const u64 g = field_generator(t), r1 = (u64)((((unsigned __int128)1) << 64) / t);
        std::vector<u64> pts(n);
        if (emu_roots_points(logn, t, pts.data())) return -1;
        u64 c = roots_coset_before(g, 0, t, r1);
        for (u32 j = 0; j < cosets; j++) {
            c = roots_mul(c, g, t, r1);
            for (size_t k = 0; k < n; k++) out[(size_t)j * n + k] = roots_value(c, pts[k], t, r1);
        }
        return 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// k_bin_roots and k_roots_mult on ONE bin, as the workgroups and the wave run them: col[rows] are the bin's coefficients mod t (the
// count is the index of the highest non-zero one), `blocks` the number of coset blocks the bin's cosets are split into (each block a
// work item of its own, with its own scaled load).  values / mult [cap]: the distinct roots in the order found and their
// multiplicities; returns how many were found, -1 (emu_last_error) on a refusal.  cap >= count.
int64_t emu_bin_roots(int logn, uint64_t t, const uint64_t *col_in, uint32_t rows, uint32_t blocks, uint64_t *values, uint32_t *mult, uint32_t cap)
{
    try {
        const size_t n = (size_t)1 << logn;
        const u32 cosets = roots_coset_count(t, n);
        int top = (int)rows - 1;
        while (top >= 0 && col_in[top] == 0) top--;
        if (top < 0) throw std::invalid_argument("the zero polynomial is not a bin");
        const u32 cnt = (u32)top;
        if (cnt >= n) throw std::invalid_argument("degree does not fit one transform");
        if (cap < cnt) throw std::invalid_argument("cap below the count");
        if (!blocks || blocks > cosets) throw std::invalid_argument("blocks out of range");
        const int T = (int)std::max<size_t>(64, n / 16);
        const EmuTables et(logn, t);
        const NttTable &tab = et.tab;
        const u64 q = tab.q, r1 = tab.r1, g = field_generator(t);
        const std::vector<u32> step = roots_step_table(g, t, n);
        std::vector<u64> pts(n), col(col_in, col_in + rows);
        if (emu_roots_points(logn, t, pts.data())) return -1;
        RootsGrid grid;
        grid.per_block = (cosets + blocks - 1) / blocks;
        grid.blocks = (cosets + grid.per_block - 1) / grid.per_block;
        u32 found = 0;
        if (cnt >= 1) {                                              // an occupied bin: the work items of k_bin_roots
            std::vector<u32> v(n);
            std::vector<u64> row(n);
            for (u32 blk = 0; blk < grid.blocks; blk++) {
                const u32 j0 = blk * grid.per_block, j1 = std::min(cosets, j0 + grid.per_block);
                u64 c = roots_coset_before(g, j0, q, r1);
                for (int tid = 0; tid < T; tid++)
                    for (int e = tid; e < (int)n; e += T) v[e] = (u32)e <= cnt ? (u32)roots_scaled_load(col[e], c, (u32)e, q, r1) : 0;
                if (blk == 0 && roots_is_zero(col[0])) roots_append(&found, values, cnt, 0);
                for (u32 j = j0; j < j1; j++) {
                    c = roots_mul(c, g, q, r1);
                    const SrcCoset ops{ v.data(), step.data() };
                    switch (logn) {
                        case 6: emu_ntt_coset<6>(row.data(), tab, T, ops); break;
                        case 8: emu_ntt_coset<8>(row.data(), tab, T, ops); break;
                        case 10: emu_ntt_coset<10>(row.data(), tab, T, ops); break;
                        case 12: emu_ntt_coset<12>(row.data(), tab, T, ops); break;
                        case 13: emu_ntt_coset<13>(row.data(), tab, T, ops); break;
                        default: throw std::invalid_argument("unsupported logn");
                    }
                    for (int tid = 0; tid < T; tid++)
                        for (int e = tid; e < (int)n; e += T)
                            if (roots_is_zero(row[e])) roots_append(&found, values, cnt, roots_value(c, pts[e], q, r1));
                }
            }
        }
        // k_roots_mult: the wave of this bin
        const u32 nf = std::min(found, cnt);
        if (nf < cnt) {
            u32 top_now = cnt;
            for (u32 base = 0; base < nf; base += ROOTS_LANES) {
                u64 r[ROOTS_LANES], b1s[ROOTS_LANES];
                bool live[ROOTS_LANES];
                for (u32 lane = 0; lane < ROOTS_LANES; lane++) {
                    live[lane] = base + lane < nf;
                    r[lane] = live[lane] ? values[base + lane] : 0;
                    u64 b0 = 0, b1 = 0;
                    for (int d = (int)cnt; d >= 0; d--) roots_deriv_step(b0, b1, r[lane], col[d], q, r1);
                    b1s[lane] = b1;
                    if (live[lane] && b1 != 0) mult[base + lane] = 1;
                }
                for (u32 l = 0; l < ROOTS_LANES; l++) {               // the ballot's bits, lowest first; lane 0 works
                    if (!(live[l] && b1s[l] == 0)) continue;
                    const u64 a = r[l];
                    u32 m = 0;
                    for (;;) {
                        u64 rem = 0;
                        for (int k = (int)top_now; k >= 0; k--) rem = roots_div_step(col[k], a, rem, q, r1);
                        if (rem != 0 || top_now == 0) break;
                        u64 sv = 0;
                        for (int k = (int)top_now; k >= 0; k--) {
                            const u64 pk = col[k];
                            col[k] = sv;
                            sv = roots_div_step(pk, a, sv, q, r1);
                        }
                        top_now--;
                        m++;
                    }
                    mult[base + l] = m;
                }
            }
        } else std::fill(mult, mult + nf, 1u);
        return (int64_t)found;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// the host end of the call (roots_expand): out[count] = the sorted multiset, or -1 with the refusal in emu_last_error
int emu_roots_expand(uint32_t slot, uint32_t count, const uint64_t *values, const uint32_t *mult, uint32_t found, uint64_t *out)
{
    try {
        std::vector<u64> v;
        roots_expand(slot, count, values, mult, found, v);
        std::copy(v.begin(), v.end(), out);
        return 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// ---- splitting and moving (bin_split.h, db_rebase.h)
uint32_t emu_split_cut(uint32_t c, uint32_t k, uint32_t p) { return split_cut(c, k, p); }
uint32_t emu_split_part_of(uint32_t c, uint32_t k, uint32_t pos) { return split_part_of(c, k, pos); }
uint32_t emu_split_capacity(uint32_t hstride) { return split_capacity(hstride); }
// the number of parts, or -1 with emu_last_error
int64_t emu_split_parts(uint32_t max_count, uint32_t limit)
{
    try { return (int64_t)split_parts(max_count, limit); } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// k_roots_split as its workgroups run it, one after the other: the launcher's arguments on host arrays (launch_roots.h: launch_roots_split,
// the zeroing of counts_out included).  *failure: SPLIT_NO_FAILURE beforehand, as on the device.  Returns 0, -1 for what the launcher refuses.
int emu_roots_split(const uint64_t *hits, const uint32_t *found, const uint32_t *mult, uint32_t hstride, const uint32_t *occ, const uint32_t *counts,
                    uint32_t n_occ, uint32_t k, uint64_t *out, const uint64_t *part_off, const uint32_t *part_stride, uint32_t *counts_out, uint32_t cstride,
                    uint64_t *failure)
{
    try {
        split_emulate(hits, found, mult, hstride, occ, counts, n_occ, k, out, part_off, part_stride, counts_out, cstride, failure);
        return 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// rebase_compatible of two parameter files: 1 compatible, 0 not (the reason in emu_last_error), -1 a file that does not load
int emu_rebase_compatible(const char *src_json, const char *dst_json)
{
    try {
        const std::string why = rebase_compatible(PSUParams::Load(src_json), PSUParams::Load(dst_json));
        g_err = why;
        return why.empty() ? 1 : 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// rebase_plan: parts [n_bundles], first [n_bundles]; cache_idx / origin [capacity].  Returns the number of output BinBundles, -1 on a
// refusal, -2 when capacity is too small.
int64_t emu_rebase_plan(const uint32_t *max_count, const uint32_t *bundle_idx, uint32_t n_bundles, uint32_t dst_max_items, uint32_t *parts, uint32_t *first,
                        uint32_t *cache_idx, uint32_t *origin, uint64_t capacity)
{
    try {
        const RebasePlan plan = rebase_plan(max_count, bundle_idx, n_bundles, dst_max_items);
        if (plan.cache_idx.size() > capacity) return -2;
        std::copy(plan.parts.begin(), plan.parts.end(), parts);
        std::copy(plan.first.begin(), plan.first.end(), first);
        std::copy(plan.cache_idx.begin(), plan.cache_idx.end(), cache_idx);
        std::copy(plan.origin.begin(), plan.origin.end(), origin);
        return (int64_t)plan.cache_idx.size();
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// place_entries (db_place.h).  counts [n_bundles][bins]; *_present [n_bundles][count]; felts [count][F].  Outputs: per entry status and
// target; state [n_bundles]; *n_new; the per-bin lists of every BinBundle, given and appended, in apsu_he_bundle_update's layout with the
// caller's stride: *_counts_out [n_bundles + n_ins][bins], *_roots_out [n_bundles + n_ins][bins][stride] (rows beyond n_bundles + *n_new
// are not written).  Returns 0; -1: a refusal (std::invalid_argument); -2: a list longer than `stride`.  Text: emu_last_error.
int emu_place_entries(uint32_t n_bundles, uint32_t bins, uint32_t F, uint64_t t, uint32_t max_items, const uint32_t *counts,
                      const unsigned char *ins_present, const unsigned char *rem_present, const uint64_t *ins_felts, const uint32_t *ins_start,
                      uint64_t n_ins, const uint64_t *rem_felts, const uint32_t *rem_start, uint64_t n_rem, uint32_t *ins_status, uint32_t *ins_target,
                      uint32_t *rem_status, uint32_t *rem_target, uint32_t *state, uint32_t *n_new, uint32_t stride, uint32_t *ins_counts_out,
                      uint64_t *ins_roots_out, uint32_t *rem_counts_out, uint64_t *rem_roots_out)
{
    try {
        PlaceInput in;
        in.n_bundles = n_bundles; in.bins = bins; in.F = F; in.max_items = max_items; in.t = t;
        in.counts = counts; in.ins_present = ins_present; in.rem_present = rem_present;
        in.ins_felts = ins_felts; in.ins_start = ins_start; in.n_ins = n_ins;
        in.rem_felts = rem_felts; in.rem_start = rem_start; in.n_rem = n_rem;
        const PlaceResult out = place_entries(in);
        std::copy(out.ins_status.begin(), out.ins_status.end(), ins_status);
        std::copy(out.ins_target.begin(), out.ins_target.end(), ins_target);
        std::copy(out.rem_status.begin(), out.rem_status.end(), rem_status);
        std::copy(out.rem_target.begin(), out.rem_target.end(), rem_target);
        std::copy(out.state.begin(), out.state.end(), state);
        *n_new = out.n_new;
        for (int kind = 0; kind < 2; kind++)
            for (size_t b = 0; b < out.ins.size(); b++) {
                const PlaceLists &l = kind ? out.rem[b] : out.ins[b];
                uint32_t *co = (kind ? rem_counts_out : ins_counts_out) + b * bins;
                uint64_t *ro = (kind ? rem_roots_out : ins_roots_out) + b * bins * (size_t)stride;
                if (l.stride > stride) { g_err = "list longer than stride"; return -2; }
                for (u32 s = 0; s < bins; s++) {
                    co[s] = l.any() ? l.counts[s] : 0;
                    for (u32 r = 0; r < co[s]; r++) ro[(size_t)s * stride + r] = l.roots[(size_t)s * l.stride + r];
                }
            }
        return 0;
    } catch (const std::invalid_argument &e) { g_err = e.what(); return -1;
    } catch (const std::exception &e) { g_err = e.what(); return -3; }
}

// k_bins_merge over A[dA + 1][n] and B[dB + 1][n] as the waves run it (bin_merge.h): one wave per (tile, block of K output rows), an explicit
// loop over its 64 lanes, the K-row window of B in slots r mod K, the walk in chunks of K steps from a multiple of K, a fold every
// `fold` steps (0: merge_fold_interval(bits(t)), the device's; the sums are 64-bit for t < 2^32 and 128-bit otherwise, as there).
// The tops come from emu_bin_counts of each input, the refusals from merge_counts without a bound on the sum.  C: [dA + dB + 1][n].
// stats (may be null): work items, folds inside the walks, longest walk in steps.  Returns 0, or -1 (emu_last_error).
int emu_bins_merge(uint64_t t_, const uint64_t *A, uint32_t dA, const uint64_t *B, uint32_t dB, uint64_t n, int K, uint32_t fold, uint64_t *C,
                   uint64_t *stats)
{
    try {
        if (K < 1 || K > 16) throw std::invalid_argument("K out of range");
        const ModulusInfo mi(t_);
        const Mod t{ t_, mi.ratio[0], mi.ratio[1] };
        const int bits = merge_bits(t_);
        const bool narrow = merge_narrow(bits);
        if (!fold) fold = merge_fold_interval(bits);
        std::vector<u32> ca(n), cb(n), sum(n);
        emu_bin_counts(A, n, dA + 1, ca.data());
        emu_bin_counts(B, n, dB + 1, cb.data());
        merge_counts(ca.data(), cb.data(), n, 0, sum.data());
        const std::vector<int> topsA = merge_tile_tops(ca.data(), n), topsB = merge_tile_tops(cb.data(), n);
        const u32 rows = dA + dB + 1, blocks = (rows + K - 1) / K;
        u64 folds = 0, longest = 0;
        for (size_t tile = 0; tile < topsA.size(); tile++)
            for (u32 blk = 0; blk < blocks; blk++) {
                const int k0 = (int)blk * K, topA = topsA[tile], topB = topsB[tile];
                const MergeWalk wk = merge_walk(k0, K, topA, topB);
                if (wk.i1 >= wk.i0) longest = std::max(longest, (u64)((wk.i1 - wk.i0) / K + 1) * K);
                for (int lane = 0; lane < MERGE_LANES; lane++) {
                    const size_t slot = tile * MERGE_LANES + lane;
                    if (slot >= n) continue;                       // (the kernel's idle lanes work on slot 0 and store nothing)
                    const u64 *colA = A + slot, *colB = B + slot;
                    u64 acc64[16] = { 0 };
                    u128p acc128[16] = {};
                    if (wk.i1 >= wk.i0) {
                        auto rowB = [&](int r) -> u64 {
                            const int rc = r < 0 ? 0 : (r > topB ? topB : r);
                            const u64 v = colB[(size_t)rc * n];
                            return r == rc ? v : 0;
                        };
                        auto rowA = [&](int i) -> u64 {
                            const u64 v = colA[(size_t)(i > wk.i1 ? wk.i1 : i) * n];
                            return i <= wk.i1 ? v : 0;
                        };
                        u64 win[16];
                        win[0] = 0;
                        for (int j = 1; j < K; j++) win[j] = rowB(k0 - wk.i0 + j);
                        u32 pending = 0;
                        for (int ib = wk.i0; ib <= wk.i1; ib += K) {
                            u64 a[16], nb[16];
                            for (int u = 0; u < K; u++) {
                                a[u] = rowA(ib + u);
                                nb[u] = rowB(k0 - ib - u);
                            }
                            for (int u = 0; u < K; u++) {
                                if (pending == fold) {
                                    for (int j = 0; j < K; j++) {
                                        if (narrow) acc64[j] = merge_fold_narrow(acc64[j], t);
                                        else acc128[j] = u128p{ merge_fold_wide(acc128[j], t), 0 };
                                    }
                                    pending = 0;
                                    if (!lane) folds++;
                                }
                                pending++;
                                win[(K - u) % K] = nb[u];
                                for (int j = 0; j < K; j++) {
                                    if (narrow) merge_mac_narrow(acc64[j], a[u], win[(j - u + K) % K]);
                                    else merge_mac_wide(acc128[j], a[u], win[(j - u + K) % K]);
                                }
                            }
                        }
                    }
                    for (int j = 0; j < K && (u32)(k0 + j) < rows; j++)
                        C[(size_t)(k0 + j) * n + slot] = narrow ? merge_fold_narrow(acc64[j], t) : merge_fold_wide(acc128[j], t);
                }
            }
        if (stats) { stats[0] = topsA.size() * (u64)blocks; stats[1] = folds; stats[2] = longest; }
        return 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

uint32_t emu_merge_fold_interval(int bits) { return merge_fold_interval(bits); }
int emu_merge_fold_exact(int bits) { return merge_fold_exact(bits) ? 1 : 0; }
int emu_merge_k() { return MERGE_K; }

// merge_counts (bin_merge.h): sum[n], or -1 with the first offending slot named in emu_last_error.  max_items 0: no bound on the sum.
int emu_merge_counts(const uint32_t *a, const uint32_t *b, uint64_t n, uint32_t max_items, uint32_t *sum)
{
    try { merge_counts(a, b, n, max_items, sum); return 0; } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// merge_steps (bin_merge.h): rows[n_bundles - 1], tops[2 (n_bundles - 1) tiles], *degree.  Returns 0, -1 for merge_counts' refusals
// (std::invalid_argument) or -3 for the logic error, the text in emu_last_error.
int emu_merge_steps(const uint32_t *counts, const uint32_t *degrees, uint32_t n_bundles, uint64_t n, uint32_t max_items, uint32_t *rows, int *tops,
                    uint32_t *degree)
{
    try {
        if (!n_bundles) throw std::invalid_argument("no BinBundle");
        const MergeSteps ms = merge_steps(counts, degrees, n_bundles, n, max_items);
        std::copy(ms.rows.begin(), ms.rows.end(), rows);
        std::copy(ms.tops.begin(), ms.tops.end(), tops);
        *degree = ms.degree;
        return 0;
    } catch (const std::invalid_argument &e) { g_err = e.what(); return -1;
    } catch (const std::exception &e) { g_err = e.what(); return -3; }
}

// k_bins_rows over poly[rows][n] as the workgroups run it (bin_rows.h): one workgroup per tile of 64 slots x 64 degrees, an explicit
// loop over its waves and their 64 lanes, the padded LDS tile between the two phases.  counts: n words (emu_bin_counts' form);
// out: at least off[bins] words, where off is rows_offsets' scan, also returned in off_out (bins + 1 words, may be null).
// Returns off[bins], or -1 (emu_last_error).
int64_t emu_bins_rows(const uint64_t *poly, uint64_t n, uint32_t rows, const uint32_t *counts, uint32_t bins, uint64_t *off_out, uint64_t *out)
{
    try {
        if (bins > n) throw std::invalid_argument("more bins than slots");
        const std::vector<u64> off = rows_offsets(counts, bins, rows);
        const std::vector<int> tops = rows_tile_tops(counts, n, bins);
        if (off_out) std::copy(off.begin(), off.end(), off_out);
        const u32 dtiles = (rows + ROWS_TILE - 1) / ROWS_TILE;
        std::vector<u64> tile(ROWS_LDS_WORDS);
        for (size_t bx = 0; bx < tops.size(); bx++)
            for (u32 by = 0; by < dtiles; by++) {
                const size_t s0 = bx * ROWS_TILE;
                const u32 d0 = by * ROWS_TILE;
                const int top = tops[bx];
                if ((int)d0 > top) continue;
                std::fill(tile.begin(), tile.end(), ~(u64)0);      // (what a live store reads was loaded: anything else would show)
                for (int wave = 0; wave < ROWS_WAVES; wave++)
                    for (int dl = wave; dl < ROWS_TILE; dl += ROWS_WAVES)
                        for (int lane = 0; lane < ROWS_TILE; lane++)
                            if (rows_load_live(d0 + dl, s0 + lane, rows, n, top)) tile[rows_lds_at(dl, lane)] = poly[(size_t)(d0 + dl) * n + s0 + lane];
                for (int wave = 0; wave < ROWS_WAVES; wave++)
                    for (int sl = wave; sl < ROWS_TILE; sl += ROWS_WAVES) {
                        const size_t s = s0 + sl;
                        if (s >= bins) break;
                        for (int lane = 0; lane < ROWS_TILE; lane++)
                            if (rows_store_live(d0 + lane, s, counts[s], bins)) out[off[s] + d0 + lane] = tile[rows_lds_at(lane, sl)];
                    }
            }
        return (int64_t)off[bins];
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// plan_compaction (db_compact.h).  counts [n_bundles][n]; group [n_bundles]; degree [n_bundles] (the first `return value` are written).
// Returns the number of groups.
int emu_plan_compaction(const uint32_t *counts, uint32_t n_bundles, uint64_t n, uint32_t max_items, uint32_t *group, uint32_t *degree)
{
    try {
        const CompactPlan plan = plan_compaction(counts, n_bundles, n, max_items);
        std::copy(plan.group.begin(), plan.group.end(), group);
        std::copy(plan.degree.begin(), plan.degree.end(), degree);
        return (int)plan.degree.size();
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// ---- the multi-device handle's rules (multi_place.h)
// place_new_unit: the slot, or -1 (emu_last_error)
int emu_place_new_unit(uint32_t bundle_idx, uint32_t bundle_idx_count, int world, const uint64_t *load)
{
    try { return place_new_unit(bundle_idx, bundle_idx_count, world, load); } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

static std::vector<RegUnit> emu_units(const int32_t *slot, const uint32_t *bundle_idx, const uint32_t *cache_idx, const uint32_t *degree, uint32_t count)
{
    std::vector<RegUnit> v(count);
    for (uint32_t i = 0; i < count; i++) { v[i].slot = slot[i]; v[i].bundle_idx = bundle_idx[i]; v[i].cache_idx = cache_idx[i]; v[i].degree = degree[i]; }
    return v;
}

// device_loads: load[world]; 0, or -1
int emu_device_loads(const int32_t *slot, const uint32_t *degree, uint32_t count, int world, uint64_t *load)
{
    try {
        std::vector<uint32_t> zero(count, 0);
        const std::vector<uint64_t> l = device_loads(emu_units(slot, zero.data(), zero.data(), degree, count), world);
        std::copy(l.begin(), l.end(), load);
        return 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// index_in_cache_order: ids[count] (the first `return value` are written), or -1: two BinBundles of the index share a cache_idx
int emu_index_in_cache_order(const uint32_t *bundle_idx, const uint32_t *cache_idx, uint32_t count, uint32_t which, int32_t *ids)
{
    try {
        std::vector<int32_t> slot(count, 0);
        std::vector<uint32_t> zero(count, 0);
        const std::vector<int> v = index_in_cache_order(emu_units(slot.data(), bundle_idx, cache_idx, zero.data(), count), which);
        std::copy(v.begin(), v.end(), ids);
        return (int)v.size();
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// merge_home of the members given by slot and cache_idx: the slot; *first = the position of the first member in cache order.  -1: no members
int emu_merge_home(const int32_t *slot, const uint32_t *cache_idx, uint32_t count, uint32_t *first)
{
    try {
        std::vector<uint32_t> zero(count, 0);
        const std::vector<RegUnit> m = emu_units(slot, zero.data(), cache_idx, zero.data(), count);
        if (first) *first = (uint32_t)merge_first(m);
        return merge_home(m);
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// registry_after.  The old registry and the appended BinBundles as four arrays each; dropped[old_count]; replaced_degree[old_count]
// (< 0: unchanged).  Outputs: new_id[old_count + n_appended] and the new registry's four arrays (capacity old_count + n_appended).
// Returns the new count, or -1 (emu_last_error).
int emu_registry_after(const int32_t *slot, const uint32_t *bundle_idx, const uint32_t *cache_idx, const uint32_t *degree, uint32_t old_count,
                       const unsigned char *dropped, const int64_t *replaced_degree, const int32_t *app_slot, const uint32_t *app_bundle_idx,
                       const uint32_t *app_cache_idx, const uint32_t *app_degree, uint32_t n_appended, int32_t *new_id, int32_t *out_slot,
                       uint32_t *out_bundle_idx, uint32_t *out_cache_idx, uint32_t *out_degree)
{
    try {
        const RegistryAfter r = registry_after(emu_units(slot, bundle_idx, cache_idx, degree, old_count),
                                               std::vector<unsigned char>(dropped, dropped + old_count),
                                               std::vector<int64_t>(replaced_degree, replaced_degree + old_count),
                                               emu_units(app_slot, app_bundle_idx, app_cache_idx, app_degree, n_appended));
        std::copy(r.new_id.begin(), r.new_id.end(), new_id);
        for (size_t i = 0; i < r.registry.size(); i++) {
            out_slot[i] = r.registry[i].slot; out_bundle_idx[i] = r.registry[i].bundle_idx;
            out_cache_idx[i] = r.registry[i].cache_idx; out_degree[i] = r.registry[i].degree;
        }
        return (int)r.registry.size();
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

} // extern "C"

// ---- the multiply-accumulate family (mac_core.h: the functions the kernels run, stepped over every lane of a launch's grid; mac_plan.h)
// A level of nl limbs whose k_mac constants are GIVEN, so that a test can pass wrong ones: per limb the modulus, the split width, the
// chunk of either form and the row width in bits (64: dense); n lays the packed rows out.
static DevLevel mac_level(int nl, const uint64_t *q, const uint32_t *shift, const uint32_t *chunk, const uint32_t *chunk_k, const uint32_t *bits, size_t n)
{
    if (nl < 1 || nl > DMAXL) throw std::invalid_argument("limbs");
    DevLevel d;
    std::memset(&d, 0, sizeof(d));
    d.L = nl;
    for (int j = 0; j < nl; j++) {
        d.q[j] = make_mod(q[j]);
        d.mac_shift[j] = shift[j]; d.mac_chunk[j] = chunk[j]; d.mac_chunk_k[j] = chunk_k[j];
        d.mac_bits[j] = bits[j];
        d.mac_row_off[j] = j ? d.mac_row_off[j - 1] + (u32)(n * bits[j - 1] / 8) : 0;
        d.mac_mask_hi[j] = mac_mask_hi_of(bits[j], (int)shift[j]);
    }
    return d;
}
template <bool KARA, bool PACKED> static void emu_mac_grid(const DevLevel &lv, const MacJob *jobs, size_t n, int njobs, int limb_slow)
{
    const unsigned gx = mac_grid(n, (size_t)njobs).gx, gl = (unsigned)lv.L, gj = (unsigned)njobs;
    const unsigned gy = limb_slow ? gj : gl, gz = limb_slow ? gl : gj;            // launch_mac's two grids
    for (unsigned bz = 0; bz < gz; bz++)
        for (unsigned by = 0; by < gy; by++)
            for (unsigned bx = 0; bx < gx; bx++)
                for (unsigned tx = 0; tx < (unsigned)EW_T; tx++) k_mac<KARA, PACKED>(&lv, jobs, n, limb_slow, bx, by, bz, tx);
}
extern "C" {

// k_mac over njobs jobs (MacJob as the device reads it, emu_mac_job_bytes) in either form and either grid order
int emu_mac(int nl, const uint64_t *q, const uint32_t *shift, const uint32_t *chunk, const uint32_t *chunk_k, const uint32_t *bits, uint64_t n,
            const void *jobs, int njobs, int kara, int packed, int limb_slow)
{
    try {
        const DevLevel lv = mac_level(nl, q, shift, chunk, chunk_k, bits, n);
        const MacJob *mj = static_cast<const MacJob *>(jobs);
        if (packed) { if (kara) emu_mac_grid<true, true>(lv, mj, n, njobs, limb_slow); else emu_mac_grid<false, true>(lv, mj, n, njobs, limb_slow); }
        else if (kara) emu_mac_grid<true, false>(lv, mj, n, njobs, limb_slow);
        else emu_mac_grid<false, false>(lv, mj, n, njobs, limb_slow);
        return 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}
int emu_mac_job_bytes() { return (int)sizeof(MacJob); }
// k_term_product over njobs TermJobs {pt, pw, out} on limb `limb`
int emu_term_product(int nl, const uint64_t *q, const uint32_t *shift, const uint32_t *chunk, const uint32_t *chunk_k, const uint32_t *bits, uint64_t n,
                     const void *jobs, uint64_t njobs, int limb, uint32_t pw_poly_stride, uint32_t out_poly_stride, int packed)
{
    try {
        const DevLevel lv = mac_level(nl, q, shift, chunk, chunk_k, bits, n);
        const TermJob *tj = static_cast<const TermJob *>(jobs);
        const size_t lanes = (n / 2 + EW_T - 1) / EW_T * EW_T;                   // launch_term_product's grid
        for (size_t u = 0; u < njobs; u++)
            for (size_t t = 0; t < lanes; t++) {
                if (packed) term_product_lane<true>(&lv, tj, njobs, n, limb, pw_poly_stride, out_poly_stride, t * 2, u);
                else term_product_lane<false>(&lv, tj, njobs, n, limb, pw_poly_stride, out_poly_stride, t * 2, u);
            }
        return 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}
// k_pack_rows / k_unpack_rows over `slots` slots of L limbs (the level's first L row widths)
int emu_pack_rows(int L, const uint32_t *bits, uint64_t n, const uint64_t *dense, void *packed, uint64_t slot_bytes, uint64_t slots, int unpack, uint64_t *dense_out)
{
    try {
        std::vector<uint64_t> q(L, 3); std::vector<uint32_t> z(L, 1);
        const DevLevel lv = mac_level(L, q.data(), z.data(), z.data(), z.data(), bits, n);
        const size_t lanes = ((unpack ? n : n * 2) + EW_T - 1) / EW_T * EW_T;     // launch_pack_rows / launch_unpack_rows
        for (unsigned by = 0; by < (unsigned)(slots * L); by++)                  // the kernels' blockIdx.y
            for (size_t t = 0; t < lanes; t++) {
                if (unpack) unpack_rows_lane(&lv, L, static_cast<const char *>(packed), slot_bytes, dense_out, n, t, by / L, (int)(by % L));
                else pack_rows_lane(&lv, L, dense, static_cast<char *>(packed), slot_bytes, n, t, by / L, (int)(by % L));
            }
        return 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}
uint32_t emu_packed_row_bits(uint64_t q) { return packed_row_bits(q); }
uint64_t emu_packed_coeff(const uint32_t *row, uint64_t c, uint32_t w) { return packed_coeff(row, c, w); }
// coefficients k, k + 1 (k even) of a row of kb-bit coefficients through the 16-byte window a lane of k_mac / k_term_product loads
void emu_packed_pair(const void *row, uint64_t k, uint32_t kb, uint64_t *out)
{
    u32 psh;
    const u32x4a4 w = ldg16_a4_nt(packed_window(row, 0, k, kb, psh));
    packed_pair((u64)w[0] | ((u64)w[1] << 32), (u64)w[2] | ((u64)w[3] << 32), psh, kb, out[0], out[1]);
}
// the rules of the modulus: out = { shift, chunk, chunk of the three-product form, that form usable }
void emu_mac_rules(uint64_t q, uint32_t *out)
{
    out[0] = (uint32_t)mac_shift_of(q); out[1] = mac_chunk_of(q); out[2] = mac_chunk_k_of(q); out[3] = mac_kara_usable(q) ? 1 : 0;
}
// mac_plan: streams [ns][11] = { pt, pw, out, cnt, pt_stride, pw_stride, pw_poly_stride, out_poly_stride, limb0, nl, packed };
// jobs (may be NULL): room for `cap` MacJobs; info = { jobs, units, mean chain length, three-product, packed, gx, limb_slow }
int emu_mac_plan(const uint64_t *streams, uint64_t ns, const uint64_t *q, int nlimbs, uint64_t n, int kara_switch, void *jobs, uint64_t cap, uint64_t *info)
{
    try {
        std::vector<MacStream> ss(ns);
        for (size_t i = 0; i < ns; i++) {
            const uint64_t *s = streams + i * 11;
            ss[i] = MacStream{ reinterpret_cast<const u64 *>(s[0]), reinterpret_cast<const u64 *>(s[1]), reinterpret_cast<u64 *>(s[2]), (u32)s[3], (u32)s[4],
                               (u32)s[5], (u32)s[6], (u32)s[7], (u32)s[8], (u32)s[9], (u32)s[10] };
        }
        const MacPlan p = mac_plan(ss, q, nlimbs, n, kara_switch);
        if (jobs) { if (p.jobs.size() > cap) throw std::invalid_argument("job buffer too small"); std::memcpy(jobs, p.jobs.data(), p.jobs.size() * sizeof(MacJob)); }
        const uint64_t v[7] = { p.jobs.size(), p.units, p.mean_cnt, p.kara, p.packed, p.grid.gx, (uint64_t)p.grid.limb_slow };
        for (int i = 0; i < 7; i++) info[i] = v[i];
        return 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

} // extern "C"

// ---- cuckoo hashing (cuckoo.h: the functions kernels_cuckoo.hip runs; model: tests/cuckoo_model.py)
extern "C" {

// tab[16][256] of location function f
void emu_cuckoo_tables(uint32_t f, uint32_t *tab) { cuckoo_tables(f, tab); }

// locs[count][H] of items [count][16] in a table of T slots
int emu_cuckoo_locations(const uint8_t *items, uint64_t count, uint32_t H, uint32_t T, uint32_t *locs)
{
    try {
        if (!H || H > CUCKOO_MAX_FUNCS || !T) throw std::invalid_argument("1 <= H <= 8 and T >= 1");
        std::vector<u32> tab(CUCKOO_TAB_WORDS);
        for (u32 f = 0; f < H; f++) {
            cuckoo_tables(f, tab.data());
            for (size_t i = 0; i < count; i++) locs[i * H + f] = cuckoo_loc(tab.data(), items + i * 16, T);
        }
        // once more as k_cuckoo_locations computes them: the staged, interleaved image of each group and cuckoo_hash_group
        std::vector<u32> tabs((size_t)H * CUCKOO_TAB_WORDS);
        for (u32 f = 0; f < H; f++) cuckoo_tables(f, tabs.data() + (size_t)f * CUCKOO_TAB_WORDS);
        const u32 G = cuckoo_group(H);
        std::vector<u32> img((size_t)G * CUCKOO_TAB_WORDS);
        for (u32 g0 = 0; g0 < H; g0 += G) {
            const u32 ng = std::min(G, H - g0);
            for (u32 idx = 0; idx < G * CUCKOO_TAB_WORDS; idx++)
                img[cuckoo_group_image(idx, G)] = idx < ng * CUCKOO_TAB_WORDS ? tabs[(size_t)g0 * CUCKOO_TAB_WORDS + idx] : 0;
            for (size_t i = 0; i < count; i++) {
                u32 w[4], x[4] = { 0, 0, 0, 0 };
                std::memcpy(w, items + i * 16, 16);
                if (G == 1) cuckoo_hash_group<1>(img.data(), w[0], w[1], w[2], w[3], x);
                else if (G == 2) cuckoo_hash_group<2>(img.data(), w[0], w[1], w[2], w[3], x);
                else cuckoo_hash_group<4>(img.data(), w[0], w[1], w[2], w[3], x);
                for (u32 g = 0; g < ng; g++)
                    if (x[g] % T != locs[i * H + g0 + g]) throw std::logic_error("the grouped hash differs from cuckoo_loc");
            }
        }
        return 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// The table rule with k_cuckoo_insert's phases as explicit loops over the items: propose, the barrier, settle.  table_idx[T],
// item_loc[count], *rounds = rounds run.  -> 0, or 1 with *unplaced = the lowest item without a slot after max_rounds and *placed = the
// slots taken (then table_idx and item_loc mean nothing), or -1.
int emu_cuckoo_insert(const uint8_t *items, const uint32_t *locs, uint64_t count, uint32_t H, uint32_t T, uint64_t max_rounds, uint32_t *table_idx,
                      uint32_t *item_loc, uint64_t *rounds, uint64_t *unplaced, uint64_t *placed)
{
    try {
        if (!H || !T || !max_rounds || max_rounds > CUCKOO_MAX_ROUNDS || count >= CUCKOO_NONE) throw std::invalid_argument("outside the rule's ranges");
        for (size_t k = 0; k < count * H; k++) if (locs[k] >= T) throw std::invalid_argument("location outside the table");
        std::vector<u64> table(T, CUCKOO_EMPTY);
        std::vector<u32> state(count, CUCKOO_ACTIVE), h(count, 0), prop(count, 0);
        u64 r = 0;
        bool more = count != 0;
        while (more && r < max_rounds) {
            for (size_t i = 0; i < count; i++) {
                if (state[i] != CUCKOO_ACTIVE) continue;
                u64 &slot = table[locs[i * H + h[i]]];
                slot = std::min(slot, cuckoo_key(max_rounds, r, (u32)i));
                prop[i] = (u32)r;
            }
            more = false;
            for (size_t i = 0; i < count; i++) {
                if (state[i] == CUCKOO_DUPLICATE) continue;
                const u64 own = cuckoo_key(max_rounds, prop[i], (u32)i), v = table[locs[i * H + h[i]]];
                const bool eq = v != own && cuckoo_items_equal(items + (size_t)cuckoo_key_item(v) * 16, items + i * 16);
                state[i] = cuckoo_settle(own, v, eq);
                if (state[i] == CUCKOO_ACTIVE) { h[i] = (h[i] + 1) % H; more = true; }
            }
            r++;
        }
        *rounds = r; *unplaced = ~(u64)0; *placed = 0;
        for (size_t i = count; i-- > 0;) { if (state[i] == CUCKOO_ACTIVE) *unplaced = i; *placed += state[i] == CUCKOO_PLACED; }
        if (*unplaced != ~(u64)0) return 1;
        for (u32 s = 0; s < T; s++) table_idx[s] = table[s] == CUCKOO_EMPTY ? CUCKOO_NONE : cuckoo_key_item(table[s]);
        for (size_t i = 0; i < count; i++) item_loc[i] = state[i] == CUCKOO_DUPLICATE ? CUCKOO_NONE : locs[i * H + h[i]];
        return 0;
    } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// the database side's grouping (cuckoo_bucket): offsets[T + 1], order[count * H]
int emu_bucket_items(const uint32_t *locs, uint64_t count, uint32_t H, uint32_t T, uint64_t *offsets, uint32_t *order, uint64_t *total)
{
    return cuckoo_bucket(locs, count, H, T, offsets, order, total) ? 0 : -1;
}

// k_query_values lane by lane: values[nb][n] of table_items [nb * items_per_bundle][16]
void emu_query_values(const uint8_t *table_items, uint32_t nb, uint32_t items_per_bundle, uint32_t F, uint32_t bpf, uint32_t item_bits, uint64_t n,
                      uint64_t *values)
{
    for (u32 b = 0; b < nb; b++)
        for (size_t p = 0; p < n; p++) {
            u32 j = 0;
            const u32 slot = query_value_slot(b, (u32)p, items_per_bundle, F, &j);
            u64 w[2] = { 0, 0 };
            if (slot != CUCKOO_NONE) std::memcpy(w, table_items + (size_t)slot * 16, 16);
            values[(size_t)b * n + p] = slot == CUCKOO_NONE ? 0 : cuckoo_item_felt(w[0], w[1], j, bpf, item_bits);
        }
}

int emu_cuckoo_lds_slots() { return (int)CUCKOO_LDS_SLOTS; }

} // extern "C"
