// The rules of ComputePowers as pure functions of the PowersDag (no HIP; like sched_policy.h, eval_plan.h and bundle_layout.h): the slot
// order and levels of a walk, whether the low and the high powers are two independent walks, how many polynomials a power and a result
// have without key switching, and where a power lies in a Powers buffer.  The Engine keeps what they return (engine.cpp's constructor)
// and decides none of it itself; tests/test_powers_sched_cpu.py holds them to a model written from the rules' one-line statements,
// through emu_powers_sched, emu_power_sizes, emu_result_size and emu_power_place of libapsu_he_hostemu.so.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "powers_dag.h"

namespace apsu_he {

constexpr uint32_t CT_SIZE_MAX = 16;                      // SEAL_CIPHERTEXT_SIZE_MAX: Ciphertext::resize throws beyond it

// One walk over the PowersDag, or over a subset of it that is closed under parents (slot order = depth, parents first, power)
struct PowersSched {
    std::vector<uint32_t> slot_power;                     // slot -> power
    std::vector<int> slot_of;                             // power -> slot (-1 if absent)
    struct Level { int s0, s1, sp; };                     // slots [s0,s1) ; [s0,sp) are parents of later nodes
    std::vector<Level> levels;
    std::vector<std::array<int, 3>> nodes;                // per non-source slot: {slot, slot_p1, slot_p2}
    std::vector<uint32_t> low_powers, high_powers;        // target powers by final form
};

// the schedule of the nodes with member[power] != 0 (indexed 0 .. the largest target power)
inline PowersSched powers_sched(const PowersDag &dag, uint32_t ps_low_degree, const std::vector<char> &member)
{
    PowersSched s;
    const uint32_t max_power = *dag.target_powers().rbegin();
    std::vector<char> is_parent(max_power + 1, 0);
    std::vector<PowersDag::PowersNode> order;
    uint32_t depth = 0;
    for (auto &kv : dag.nodes()) {
        const PowersDag::PowersNode &nd = kv.second;
        if (!member[nd.power]) continue;
        order.push_back(nd);
        depth = std::max(depth, nd.depth);
        if (!nd.is_source()) { is_parent[nd.parents.first] = 1; is_parent[nd.parents.second] = 1; }
    }
    std::stable_sort(order.begin(), order.end(), [&](const auto &a, const auto &b) {
        if (a.depth != b.depth) return a.depth < b.depth;
        if (is_parent[a.power] != is_parent[b.power]) return is_parent[a.power] > is_parent[b.power];
        return a.power < b.power;
    });
    s.slot_of.assign(max_power + 1, -1);
    s.levels.assign(depth + 1, PowersSched::Level{ 0, 0, 0 });   // (a depth without a node of this subset stays the empty range at 0)
    for (size_t i = 0; i < order.size(); i++) {
        s.slot_power.push_back(order[i].power);
        s.slot_of[order[i].power] = (int)i;
        PowersSched::Level &lv = s.levels[order[i].depth];
        if (!lv.s1) lv.s0 = lv.sp = (int)i;
        lv.s1 = (int)i + 1;
        if (is_parent[order[i].power]) lv.sp = (int)i + 1;
    }
    for (size_t i = 0; i < order.size(); i++)
        if (!order[i].is_source())
            s.nodes.push_back({ (int)i, s.slot_of[order[i].parents.first], s.slot_of[order[i].parents.second] });
    for (uint32_t p : dag.target_powers()) {
        if (!member[p]) continue;
        if (!ps_low_degree || p <= ps_low_degree) s.low_powers.push_back(p);
        else s.high_powers.push_back(p);
    }
    return s;
}

// The whole DAG's schedule and, where the walk splits, the two halves'.
// The powers that stay at the low level and the Paterson-Stockmeyer high powers usually descend from different
// query powers (all four reference parameter sets).  Then ComputePowers is two independent chains: the second one
// runs on its own stream, next to the first and to the BinBundle inner products that only need the low powers.
struct PowersScheds {
    PowersSched all, low, high;                           // low, high: empty unless split_ok
    bool split_ok = false;                                // the low-power and high-power halves of the PowersDag share no node
};
inline PowersScheds powers_scheds(const PowersDag &dag, uint32_t ps_low_degree)
{
    PowersScheds r;
    const auto &nodes = dag.nodes();
    const uint32_t max_power = *dag.target_powers().rbegin();
    r.all = powers_sched(dag, ps_low_degree, std::vector<char>(max_power + 1, 1));
    if (r.all.high_powers.empty() || r.all.low_powers.empty() || dag.depth() == 0) return r;
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
    const auto ml = closure(r.all.low_powers), mh = closure(r.all.high_powers);
    for (uint32_t p = 0; p <= max_power; p++) if (ml[p] && mh[p]) return r;
    r.low = powers_sched(dag, ps_low_degree, ml);
    r.high = powers_sched(dag, ps_low_degree, mh);
    r.split_ok = true;
    return r;
}

// Polynomials per target power: 2 with key switching; without it nothing is relinearised (receiver_osn.cpp:416,430-432) and a
// product has size(parent1) + size(parent2) - 1.  sched: the whole DAG's.
struct PowerSizes {
    std::vector<uint32_t> size;                           // index = power; 0 = no target
    bool products = false;                                // no key switching AND the PowersDag has products
    bool oversize = false;                                // some product exceeds CT_SIZE_MAX polynomials: ComputePowers throws like SEAL's multiply
    uint32_t stored = 2;                                  // polynomials stored per power (largest size, rounded up to even)
};
inline PowerSizes power_sizes(const PowersSched &sched, bool using_keyswitching, uint32_t dag_depth)
{
    PowerSizes z;
    z.size.assign(sched.slot_of.size(), 0);
    for (uint32_t p : sched.slot_power) z.size[p] = 2;
    z.products = !using_keyswitching && dag_depth > 0;
    if (!z.products) return z;
    uint32_t widest = 2;
    for (const auto &nd : sched.nodes) {                  // slot order: parents come first
        const uint32_t a = z.size[sched.slot_power[nd[1]]], b = z.size[sched.slot_power[nd[2]]];
        const uint32_t sz = std::min<uint32_t>(a + b - 1, 2 * CT_SIZE_MAX);        // (kept finite; anything above the limit throws)
        z.size[sched.slot_power[nd[0]]] = sz;
        widest = std::max(widest, sz);
    }
    z.oversize = widest > CT_SIZE_MAX;
    z.stored = (std::min(widest, CT_SIZE_MAX) + 1) & ~1u;
    return z;
}

// size of BatchedPlaintextPolyn::eval / eval_patstock's result for a BinBundle of this degree (bin_bundle.cpp:132-134 starts at
// size 2, :238-240 at size 3); values above CT_SIZE_MAX mean SEAL throws inside the evaluation
inline uint32_t result_size_for(const PowerSizes &sizes, uint32_t ps_low_degree, uint32_t degree, bool using_keyswitching)
{
    if (using_keyswitching) return 2;
    const uint32_t ps = ps_low_degree, h = ps + 1;
    auto sz = [&](uint32_t p) { return p < sizes.size.size() ? sizes.size[p] : 0u; };
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

// the largest result_size_for over the degrees a BinBundle can have = polynomials per row of eval_bundles' output
// (degrees whose evaluation SEAL refuses do not count: eval_bundles refuses them too)
inline uint32_t result_polys(const PowerSizes &sizes, uint32_t ps_low_degree, bool using_keyswitching, uint32_t max_items_per_bin)
{
    uint32_t polys = 2;
    if (!using_keyswitching)                                 // (eval_patstock alone already leaves three polynomials)
        for (uint32_t deg = 0; deg <= max_items_per_bin; deg++) {
            const uint32_t r = result_size_for(sizes, ps_low_degree, deg, using_keyswitching);
            if (r <= CT_SIZE_MAX) polys = std::max(polys, r);
        }
    return polys;
}

// where a power lies in a Powers buffer that holds n_low low and n_high high powers: the half and the index in it
struct PowerPlace { bool low; uint32_t idx; };
inline PowerPlace power_place(uint32_t ps_low_degree, uint32_t power, uint32_t n_low, uint32_t n_high)
{
    const uint32_t ps = ps_low_degree;
    if (!ps || power <= ps) {
        if (power < 1 || power > n_low) throw std::invalid_argument("power not available");
        return PowerPlace{ true, power - 1 };
    }
    if (power % (ps + 1) != 0 || power / (ps + 1) > n_high) throw std::invalid_argument("power not available");
    return PowerPlace{ false, power / (ps + 1) - 1 };
}

} // namespace apsu_he
