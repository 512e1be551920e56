// The Engine's BinBundle evaluation: BatchedPlaintextPolyn::eval (receiver/apsu/bin_bundle.cpp:106-174) and eval_patstock
// (bin_bundle.cpp:192-360), by the plan of eval_plan.h.  Exact (rounding-free) steps are batched / re-associated freely; every
// rounding step is applied per term exactly where the reference applies it (SURVEY.md §2.4 note N1).
#include "engine_impl.h"
#include "eval_plan.h"

namespace apsu_he {

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
// profiles/r03_eval_pipeline.txt; the code is in git history at 22dbbd1, the engine.cpp of that commit, lines 1600-1745.)
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
    const int rawf = behz_unrolled(h.L, h.nB) ? NTT_MAP_RAW : 0;
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
    if (pw.polys != sizes_.stored) throw std::invalid_argument("ciphertext powers do not belong to this context");
    if (sizes_.products || result_polys_ > 2) {                        // every BinBundle of such a set: the rows are result_polys_ polynomials apart
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

} // namespace apsu_he
