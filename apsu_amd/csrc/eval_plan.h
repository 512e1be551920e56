// The form decisions of one chunk of the Paterson-Stockmeyer evaluation (Engine::eval_patstock), as one pure function of a small state:
// which inverse transforms are RAW and which consumer absorbs their twist, which finish the products take, where the sums of the
// coefficient-form products run, which form the i = 0 block takes, and what moves to the side lane.  No HIP in here:
// Engine::eval_patstock fills the state, ps_tables / ps_run execute the plan; tests/test_host_logic.py enumerates the states through
// the CPU emulation library and holds the plan to its invariants -- above all that a RAW transform (NTT_MAP_RAW: no twist, no final
// reduction) is planned exactly where the kernel that takes the twist into its own constants is planned too.
#pragma once
#include <cstddef>
#include <cstdint>

namespace apsu_he {

// the unrolled BEHZ kernels (k_behz_ext2, k_behz_finish2, k_behz_finish_sum<TL, true>: Shoup-form matrices, RAW input) exist for this level
constexpr bool behz_unrolled(int L, int nB) { return L == nB && L <= 3; }

struct EvalState {
    int low, high;            // chain index of the low / high powers (low >= high: Engine::compute_powers)
    int L, nB;                // of the high level
    uint32_t l;               // ps_low_degree (> 1 for every Paterson-Stockmeyer BinBundle)
    uint64_t q_last;          // last prime of the low level
    uint64_t q_widest;        // widest prime of the high level
    int Bs, max_terms;        // BinBundles of the batch (>= 1), the most inner polynomials of one of them
    bool high_in_flight;      // the high powers are still being computed on the second stream (Powers::high_async && high_ready)
    bool eval_side, prof_on, force_per_term, fuse_tensor, fuse_tail;   // the engine's switches of the same names
    bool lane2, on_lane0;     // the side lane exists; the evaluation runs on the main lane
};
enum CfPlace {
    CF_WITH_MAC = 0,          // with the main multiply-accumulate (the high powers are complete)
    CF_SIDE_LANE = 1,         // on the side lane, behind high_ready
    CF_BEHIND_HIGH_READY = 2  // on the main stream behind its wait for high_ready, next to the products
};
enum I0Form {
    I0_SIDE = 0,              // launch_i0_finish on the side lane
    I0_SSUM = 1,              // no limb is dropped: the sum as it is
    I0_FINISH_MAIN = 2,       // launch_i0_finish on the main stream
    I0_GENERAL = 3            // every term switched down on its own, then add_many
};
struct EvalPlan {
    bool i0_fast, need_vlast, raw_drop, raw_i0, fused_drop, summed, side, side_i0, wait_high_ready, fuse_tensor, fuse_tail;
    int cf;                   // CfPlace
    int i0;                   // I0Form
};

inline EvalPlan plan_eval(const EvalState &s)
{
    EvalPlan p{};
    const int Lh = s.high + 1;
    // i = 0 block (:314-324): every term C^j (.) a_j is INTT'd and rounded to the high level ON ITS OWN before
    // the sum (note N1).  With one dropped limb the sum of the rounded terms is
    //   (sum_j c_j[m] + l*half - sum_j ((c_j[last] + half) mod q_last)) * q_last^-1  mod q_m,
    // where the first sum is exact and may be taken in the NTT domain.  So only the LAST limb of each term
    // needs its own inverse transform (2 per term instead of 2*L_low), bit-identical to the reference.
    p.i0_fast = (s.low - s.high <= 1) && ((unsigned __int128)(s.l + 1) * s.q_last < ((unsigned __int128)1 << 64));
    p.need_vlast = p.i0_fast && s.low > s.high;
    // RAW inverse transforms (no twist, no final reduction) where the consumer's own constants absorb the twist:
    // the inner polynomials when the fused drop + extension kernel takes them, the i = 0 block's sums and last limbs
    p.raw_drop = s.low == s.high + 1 && behz_unrolled(s.L, s.nB);
    p.raw_i0 = p.need_vlast;
    // a single drop is folded into the extension's pass where that kernel exists: the one consumer of the RAW inner polynomials
    // (launch_drop_behz_ext decides by the same behz_unrolled; Engine::ps_drop_ext throws if it declines)
    p.fused_drop = p.raw_drop;
    // high powers still in flight on the second stream (split ComputePowers): everything that needs only the low
    // powers goes first, the cf products (which read the high powers) come later
    p.wait_high_ready = s.high_in_flight;
    // Side lane (round 4).  Two pieces of the evaluation hang off nothing that follows on the main stream: the sums of the
    // coefficient-form products (they read the high powers and the database, :328-337) and the i = 0 block's finish (it reads the
    // inverse transforms of the merged launch).  Both are launches that cannot fill the chip (224 workgroups of 28-term chains; one pass
    // over the per-term last limbs) and used to sit in the tail of the main stream, where nothing could hide them.  They run on a
    // third stream (lane 2; the first of them waits for the high-power chain's event) next to the drop / extension / transform
    // launches, and the epilogue waits for them.  (With pipelined queries the next query's ComputePowers fills the same holes and the
    // lane is level, profiles/r04_ab_eval_side.txt; it still serves a query that runs alone.)
    p.side = s.eval_side && s.high_in_flight && !s.prof_on && p.i0_fast && s.low != s.high && s.lane2 && s.on_lane0;
    // (the i = 0 finish only while it is small: 256M-4096's reads 4 GB of per-term limbs, a bandwidth-bound pass that gains nothing
    //  from running next to the transforms -- measured +0.9 % there, -1.2 % at 16M-4096, -4.2 % on its N = 8 shard; profiles/r04_ab_eval_side.txt)
    // Round 5: with the finish, the i = 0 block's per-term products and THEIR inverse transforms leave the main stream too -- they feed
    // only that finish -- so the main chain behind k_mac starts with the inner polynomials alone: -0.017 ms (-0.5 %) on the latency of
    // the 16M-4096 query over four order-balanced A/B runs, -1.7 % on the N = 8 shard, same bits (profiles/r05_ab_side_term_product.txt).
    // (That was a flag of its own, side_tp = side_i0 && "there are term products" && need_vlast: side gives i0_fast && low != high, and
    //  low >= high, Bs >= 1, l > 1 hold in every state the engine reaches, so the two never differed.)
    p.side_i0 = p.side && (size_t)s.Bs * s.l <= 4096;
    p.cf = !s.high_in_flight ? CF_WITH_MAC : p.side ? CF_SIDE_LANE : CF_BEHIND_HIGH_READY;
    p.i0 = p.side_i0 ? I0_SIDE : p.i0_fast && s.low == s.high ? I0_SSUM : p.i0_fast ? I0_FINISH_MAIN : I0_GENERAL;
    // The products of one BinBundle are summed (:273,303).  Each keeps its own rounding (note N1), but only
    // the q limbs are needed per term for that: the Bsk limbs are summed in the NTT domain by the tensor
    // kernel and finished once per BinBundle (see behz_finish_coeff).  Bit-identical, 6 instead of 15
    // inverse transforms per term at L = 2.
    // the summed finish adds per-term canonical residues of EVERY q limb as plain integers: the widest limb bounds it
    p.summed = !s.force_per_term && Lh <= 4 && (unsigned __int128)s.max_terms * s.q_widest < ((unsigned __int128)1 << 63);
    p.fuse_tensor = s.fuse_tensor;
    p.fuse_tail = s.fuse_tail;
    return p;
}

} // namespace apsu_he
