// CPU emulation, the host's rules: parameters, device constant blocks, the powers' graph and its schedules, scheduling, the evaluation's forms, the stored
// layout of a BinBundle, the transform's launch form, the switches.  No kernel code in here: pure functions of the host, enumerated by tests.
#include <cstring>
#include <set>
#include <stdexcept>
#include <vector>

#include "emu_common.h"
#include "bundle_layout.h"
#include "dev_consts.h"
#include "eval_plan.h"
#include "params.h"
#include "powers_dag.h"
#include "powers_sched.h"
#include "sched_policy.h"

using namespace apsu_he;

extern "C" {

const char *emu_last_error() { return g_err.c_str(); }

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
    return guarded([&]() -> int {
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
    });
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
    return guarded([&]() -> int64_t {
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
    });
}
// sizeof NttTable, DevLevel, DevKey, then DMAXL, DMAXB (the test's mirror of the layouts checks itself against these)
void emu_dev_layout(uint64_t *out) { out[0] = sizeof(NttTable); out[1] = sizeof(DevLevel); out[2] = sizeof(DevKey); out[3] = DMAXL; out[4] = DMAXB; }

// read_switches() under the caller's environment: two_stream_default, eval_side, packed_rows, eval_ws_bytes, arena_bytes, force_per_term,
// mac_kara, seed_expand_host, fuse_tail, ntt_latency_limbs (signed values as int64).  Ten values: callers size their buffer for ten, so a
// switch added later gets an entry of its own below.
void emu_switches(int64_t *out)
{
    const EngineSwitches s = read_switches();
    const int64_t v[10] = { s.two_stream_default, s.eval_side, s.packed_rows, (int64_t)s.eval_ws_bytes, (int64_t)s.arena_bytes, s.force_per_term,
                            s.mac_kara, s.seed_expand_host, s.fuse_tail, (int64_t)s.ntt_latency_limbs };
    for (int i = 0; i < 10; i++) out[i] = v[i];
}
// the switches added since: out[0] = seed_rej_cap (APSU_HE_SEED_REJ_CAP as read; a context refuses a value outside 1 .. SEED_REJ_CAP).
// Returns their number (the first `cap` are written).
int emu_switches_more(int64_t *out, int cap)
{
    const EngineSwitches s = read_switches();
    const int64_t v[1] = { (int64_t)s.seed_rej_cap };
    for (int i = 0; i < 1 && i < cap; i++) out[i] = v[i];
    return 1;
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

// The rules of ComputePowers (powers_sched.h), for tests/test_powers_sched_cpu.py.  Every call configures the PowersDag of the given
// sets itself and returns -1 where that fails (or a rule refuses: emu_last_error).
static PowersDag dag_of(const uint32_t *sources, int ns, const uint32_t *targets, int nt)
{
    PowersDag d;
    if (!d.configure(std::set<uint32_t>(sources, sources + ns), std::set<uint32_t>(targets, targets + nt))) throw std::invalid_argument("PowersDag::configure failed");
    return d;
}
// which: 0 the whole DAG's schedule, 1 the low half's, 2 the high half's (both empty unless the walk splits).  out = split_ok, then each
// list behind its length: slot_power, slot_of, levels (s0, s1, sp each), nodes (slot, parent slots each), low_powers, high_powers.
// Returns the words of `out` (the first `cap` are written).
int emu_powers_sched(const uint32_t *sources, int ns, const uint32_t *targets, int nt, uint32_t ps_low_degree, int which, int64_t *out, int cap)
{
    return guarded([&]() -> int {
        const PowersScheds r = powers_scheds(dag_of(sources, ns, targets, nt), ps_low_degree);
        const PowersSched &s = which == 0 ? r.all : which == 1 ? r.low : r.high;
        std::vector<int64_t> v{ r.split_ok };
        auto put = [&](const auto &list) { v.push_back((int64_t)list.size()); for (auto x : list) v.push_back((int64_t)x); };
        put(s.slot_power); put(s.slot_of);
        v.push_back((int64_t)s.levels.size());
        for (const PowersSched::Level &l : s.levels) v.insert(v.end(), { l.s0, l.s1, l.sp });
        v.push_back((int64_t)s.nodes.size());
        for (const auto &nd : s.nodes) v.insert(v.end(), { nd[0], nd[1], nd[2] });
        put(s.low_powers); put(s.high_powers);
        for (size_t i = 0; i < v.size() && (int)i < cap; i++) out[i] = v[i];
        return (int)v.size();
    });
}
// out = products, oversize, stored, then size[0 .. the largest target power]
int emu_power_sizes(const uint32_t *sources, int ns, const uint32_t *targets, int nt, uint32_t ps_low_degree, int using_keyswitching, uint32_t *out, int cap)
{
    return guarded([&]() -> int {
        const PowersDag d = dag_of(sources, ns, targets, nt);
        const PowerSizes z = power_sizes(powers_scheds(d, ps_low_degree).all, using_keyswitching != 0, d.depth());
        std::vector<uint32_t> v{ z.products, z.oversize, z.stored };
        v.insert(v.end(), z.size.begin(), z.size.end());
        for (size_t i = 0; i < v.size() && (int)i < cap; i++) out[i] = v[i];
        return (int)v.size();
    });
}
// out = result_polys, then result_size_for(degree) for degree = 0 .. max_items_per_bin
int emu_result_size(const uint32_t *sources, int ns, const uint32_t *targets, int nt, uint32_t ps_low_degree, int using_keyswitching,
                    uint32_t max_items_per_bin, uint32_t *out, int cap)
{
    return guarded([&]() -> int {
        const PowersDag d = dag_of(sources, ns, targets, nt);
        const bool ks = using_keyswitching != 0;
        const PowerSizes z = power_sizes(powers_scheds(d, ps_low_degree).all, ks, d.depth());
        std::vector<uint32_t> v{ result_polys(z, ps_low_degree, ks, max_items_per_bin) };
        for (uint32_t deg = 0; deg <= max_items_per_bin; deg++) v.push_back(result_size_for(z, ps_low_degree, deg, ks));
        for (size_t i = 0; i < v.size() && (int)i < cap; i++) out[i] = v[i];
        return (int)v.size();
    });
}
// out = low, idx; -1 where the power is refused ("power not available")
int emu_power_place(uint32_t ps_low_degree, uint32_t power, uint32_t n_low, uint32_t n_high, uint32_t *out)
{
    return guarded([&]() -> int {
        const PowerPlace at = power_place(ps_low_degree, power, n_low, n_high);
        out[0] = at.low; out[1] = at.idx;
        return 0;
    });
}

int emu_create_powers_set(uint32_t ps_low, uint32_t target, uint32_t *out, int cap)
{
    return guarded([&]() -> int {
        auto s = create_powers_set(ps_low, target);
        int i = 0;
        for (uint32_t p : s) { if (i < cap) out[i] = p; i++; }
        return i;
    });
}

// level constants flattened for diffing against the oracle (test_constants)
int emu_level_constants(uint64_t n, const uint64_t *q, int k, uint64_t t, int chain_idx, uint64_t *out, int cap)
{
    return guarded([&]() -> int {
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
    });
}

} // extern "C"
