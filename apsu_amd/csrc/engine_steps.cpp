// One element-wise kernel at a time on caller-chosen words (Engine::debug_run_step; include/apsu_he.h: apsu_he_debug_run_step).
// A step copies host arrays in the layout device.h documents for its launcher, builds the job structs, calls THE launch_* function the
// engine calls with this context's own DevLevel / DevKey blocks -- so the launcher's template dispatch is part of what runs --
// synchronises and copies the result back.  Whatever the launcher's input contract (device.h) does not admit is refused before
// anything is launched: sizes, levels, a RAW form the launcher does not have, a term count beyond the bound the engine checks on the
// host, and a word that is not a canonical residue where the contract asks for one.  For the tests; nothing on the query path calls it.
#include "engine_impl.h"
#include "eval_plan.h"

#include <string>

namespace apsu_he {

namespace {

[[noreturn]] void refuse(const std::string &why) { throw std::invalid_argument("debug_run_step: " + why); }
void need(bool ok, const char *why) { if (!ok) refuse(why); }

// rows[r][n] with row r reduced modulo mods[r % mods.size()]
void check_canonical(const u64 *x, size_t rows, const std::vector<u64> &mods, size_t n, const char *what)
{
    for (size_t r = 0; r < rows; r++) {
        const u64 m = mods[r % mods.size()], *row = x + r * n;
        u64 bad = 0;
        for (size_t k = 0; k < n; k++) bad |= (u64)(row[k] >= m);
        if (bad) refuse(std::string(what) + " holds a word that is not a canonical residue of its limb");
    }
}

} // namespace

void Engine::debug_run_step(const StepArgs &a)
{
    Enter g(this);
    TIER1_SLOTS();
    if (a.step >= STEP_ADD) { debug_run_misc_step(a); return; }               // the launchers no other family reaches
    if (a.step >= STEP_BUCKET_COUNT) { debug_run_bucket_step(a); return; }    // the grouping by location: no chain level
    if (a.step == STEP_ENTRIES_SCATTER) { debug_run_db_step(a); return; }     // (a database step numbered behind the multiply-accumulate family)
    if (a.step >= STEP_MAC_INFO) { debug_run_mac_step(a); return; }           // the multiply-accumulate family and the packed rows
    if (a.step >= STEP_SEED_EXPAND) { debug_run_query_step(a); return; }      // the querier's side and the decryption
    if (a.step == STEP_ROOTS_SPLIT) { debug_run_db_step(a); return; }         // (a database step numbered behind the transforms)
    if (a.step >= STEP_NTT_INFO) { debug_run_ntt_step(a); return; }          // the transforms: a map of the caller's, no chain level
    if (a.step >= STEP_POLYN_WITH_ROOTS) { debug_run_db_step(a); return; }   // the mod-t kernels of a resident database: no chain level
    check_level(a.chain_idx);
    const LevelConstants &h = hlevel(a.chain_idx);
    const size_t n = hp_.n;
    const int L = h.L, nB = h.nB, nBsk = nB + 1, E = L + nBsk, K = hp_.K;
    const bool raw = a.flags & STEP_RAW, flag2 = a.flags & STEP_ACCUMULATE, store = a.flags & STEP_STORE, with_key = a.flags & STEP_KEY;
    const bool unrolled = behz_unrolled(L, nB);
    const std::vector<u64> q(h.q.begin(), h.q.end());
    std::vector<u64> bsk(h.B.begin(), h.B.end());
    bsk.push_back(h.m_sk);
    std::vector<u64> ext = q;
    ext.insert(ext.end(), bsk.begin(), bsk.end());
    const std::vector<u64> tmod{ hp_.t };
    const size_t batch = a.batch > 0 ? (size_t)a.batch : 0, polys = a.polys > 0 ? (size_t)a.polys : 0, terms = a.terms > 0 ? (size_t)a.terms : 0;

    if (a.step == STEP_LEVEL_INFO) {
        // L, nB, unrolled, K, q_0 .., B_0 .., m_sk, special prime (0 without key switching), irrelevant_bit_count
        const size_t w = 4 + (size_t)L + nBsk + 2;
        need(a.out[0] && a.out_words[0] >= w, "level_info: out[0] too small");
        u64 *o = a.out[0];
        *o++ = (u64)L; *o++ = (u64)nB; *o++ = unrolled ? 1 : 0; *o++ = (u64)K;
        for (u64 v : q) *o++ = v;
        for (u64 v : bsk) *o++ = v;
        *o++ = hp_.using_keyswitching ? hp_.key_q[K - 1] : 0;
        *o++ = (u64)hp_.irrelevant_bit_count;
        return;
    }

    need(batch >= 1 && batch <= 64, "batch out of range (1 .. 64)");
    auto in_is = [&](int i, size_t words, const char *what) { if (!a.in[i] || a.in_words[i] != words) refuse(std::string(what) + ": wrong size"); };
    auto out_is = [&](int i, size_t words, const char *what) { if (!a.out[i] || a.out_words[i] != words) refuse(std::string(what) + ": wrong size"); };
    auto canon = [&](int i, const std::vector<u64> &mods, const char *what) { check_canonical(a.in[i], a.in_words[i] / n, mods, n, what); };
    auto canon_out = [&](int i, const std::vector<u64> &mods, const char *what) { check_canonical(a.out[i], a.out_words[i] / n, mods, n, what); };

    std::vector<FinishJob> fin;
    std::vector<FinishSumJob> fsum;
    std::vector<TensorJob> tj;
    std::vector<TensorConvJob> tcj;
    std::vector<TensorSumJob> tsj;
    std::vector<CtJob> cj;
    std::vector<SumJob> sj;
    std::vector<PlainJob> pj;
    std::vector<I0Job> ij;
    std::vector<EpiJob> ej;
    std::vector<unsigned char> flags8;

    WITH_ARENA({
        fin.clear(); fsum.clear(); tj.clear(); tcj.clear(); tsj.clear(); cj.clear(); sj.clear(); pj.clear(); ij.clear(); ej.clear();   // a retry with a larger arena starts over
        auto up = [&](const u64 *src, size_t words) {
            u64 *d = ws(words);
            HIP_CHECK(hipMemcpyAsync(d, src, words * sizeof(u64), hipMemcpyHostToDevice, st_));
            return d;
        };
        auto up_in = [&](int i) { return up(a.in[i], a.in_words[i]); };
        auto down = [&](int i, const u64 *src) { HIP_CHECK(hipMemcpyAsync(a.out[i], src, a.out_words[i] * sizeof(u64), hipMemcpyDeviceToHost, st_)); };
        // job tables live in the arena for the length of the call (the host vectors outlive the copy: the call ends with a sync)
        auto jobs = [&](const auto &v) {
            using T = typename std::decay_t<decltype(v)>::value_type;
            T *d = ws_as<T>(v.size());
            HIP_CHECK(hipMemcpyAsync(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st_));
            return static_cast<const T *>(d);
        };

        switch (a.step) {
        case STEP_BEHZ_EXT: {
            need(polys >= 1 && polys <= 16, "behz_ext: polys out of range");
            need(!raw, "behz_ext: launch_behz_ext has no RAW form");
            in_is(0, batch * polys * L * n, "behz_ext: in[0] [batch][polys][L][n]");
            out_is(0, batch * polys * E * n, "behz_ext: out[0] [batch][polys][E][n]");
            canon(0, q, "behz_ext: in[0]");
            u64 *o = ws(a.out_words[0]);
            launch_behz_ext(dlevel(a.chain_idx), L, nB, up_in(0), polys * L * n, (int)polys, o, n, (int)batch, st_);
            down(0, o);
        } break;
        case STEP_DROP_BEHZ_EXT: {
            need(polys >= 1 && polys <= 16, "drop_behz_ext: polys out of range");
            need(a.chain_idx + 1 <= hp_.first_chain_idx, "drop_behz_ext: there is no level above chain_idx to drop from");
            need(unrolled, "drop_behz_ext: launch_drop_behz_ext exists for the unrolled sizes only (L == nB <= 3)");
            in_is(0, batch * polys * (L + 1) * n, "drop_behz_ext: in[0] [batch][polys][L + 1][n]");
            out_is(0, batch * polys * E * n, "drop_behz_ext: out[0] [batch][polys][E][n]");
            if (!raw) canon(0, hlevel(a.chain_idx + 1).q, "drop_behz_ext: in[0]");
            u64 *o = ws(a.out_words[0]);
            if (!launch_drop_behz_ext(dlevel(a.chain_idx), L, nB, up_in(0), polys * (L + 1) * n, (int)polys, o, n, (int)batch, st_, raw))
                throw std::logic_error("debug_run_step: launch_drop_behz_ext declined an unrolled level");
            down(0, o);
        } break;
        case STEP_TENSOR: {
            in_is(0, batch * 2 * E * n, "tensor: in[0] [batch][2][E][n]");
            in_is(1, batch * 2 * E * n, "tensor: in[1] [batch][2][E][n]");
            out_is(0, batch * 3 * E * n, "tensor: out[0] [batch][3][E][n]");
            canon(0, ext, "tensor: in[0]");
            canon(1, ext, "tensor: in[1]");
            const u64 *x = up_in(0), *y = up_in(1);
            u64 *o = ws(a.out_words[0]);
            for (size_t b = 0; b < batch; b++) tj.push_back(TensorJob{ x + b * 2 * E * n, y + b * 2 * E * n, o + b * 3 * E * n });
            launch_tensor(dlevel(a.chain_idx), jobs(tj), n, (int)batch, st_);
            down(0, o);
        } break;
        case STEP_TENSOR_CONV: {
            const size_t sa = polys, sb = terms;
            need(sa >= 1 && sb >= 1 && sa + sb - 1 <= CT_SIZE_MAX, "tensor_conv: sizes out of range (polys = sa, terms = sb, sa + sb - 1 <= 16)");
            in_is(0, batch * sa * E * n, "tensor_conv: in[0] [batch][sa][E][n]");
            in_is(1, batch * sb * E * n, "tensor_conv: in[1] [batch][sb][E][n]");
            out_is(0, batch * (sa + sb - 1) * E * n, "tensor_conv: out[0] [batch][sa + sb - 1][E][n]");
            canon(0, ext, "tensor_conv: in[0]");
            canon(1, ext, "tensor_conv: in[1]");
            const u64 *x = up_in(0), *y = up_in(1);
            u64 *o = ws(a.out_words[0]);
            for (size_t b = 0; b < batch; b++) tcj.push_back(TensorConvJob{ x + b * sa * E * n, y + b * sb * E * n, o + b * (sa + sb - 1) * E * n, (int)sa, (int)sb });
            launch_tensor_conv(dlevel(a.chain_idx), jobs(tcj), n, (int)batch, st_);
            down(0, o);
        } break;
        case STEP_TENSOR_SUM: {
            need(terms >= 1 && terms <= 4096, "tensor_sum: terms out of range");
            need(a.e0 == 0 || a.e0 == L, "tensor_sum: e0 is 0 (every limb) or L (the Bsk sums alone)");
            in_is(0, batch * terms * 2 * E * n, "tensor_sum: in[0] [batch][terms][2][E][n]");
            in_is(1, batch * terms * 2 * E * n, "tensor_sum: in[1] [batch][terms][2][E][n]");
            if (a.e0 == 0) out_is(0, batch * terms * 3 * L * n, "tensor_sum: out[0] [batch][terms][3][L][n]");
            out_is(1, batch * 3 * nBsk * n, "tensor_sum: out[1] [batch][3][nBsk][n]");
            canon(0, ext, "tensor_sum: in[0]");
            canon(1, ext, "tensor_sum: in[1]");
            const u64 *x = up_in(0), *y = up_in(1);
            u64 *dq = a.e0 == 0 ? ws(a.out_words[0]) : nullptr, *bs = ws(a.out_words[1]);
            for (size_t b = 0; b < batch; b++)
                tsj.push_back(TensorSumJob{ x + b * terms * 2 * E * n, y + b * terms * 2 * E * n, dq ? dq + b * terms * 3 * L * n : nullptr, bs + b * 3 * nBsk * n, (int)terms, 0 });
            launch_tensor_sum(dlevel(a.chain_idx), E, jobs(tsj), n, (int)batch, a.e0, st_);
            if (dq) down(0, dq);
            down(1, bs);
        } break;
        case STEP_BEHZ_FINISH: {
            need(terms >= 1 && terms <= 4096, "behz_finish: terms out of range");
            in_is(0, batch * terms * 3 * E * n, "behz_finish: in[0] [batch][terms][3][E][n]");
            out_is(0, batch * 3 * L * n, "behz_finish: out[0] [batch][3][L][n]");
            if (!unrolled) canon(0, ext, "behz_finish: in[0] (a level with the generic finish)");      // the unrolled finish takes RAW words
            else need(raw, "behz_finish: the unrolled finish (L == nB <= 3) takes RAW input only");
            if (!unrolled) need(!raw, "behz_finish: the generic finish has no RAW form");
            if (flag2) canon_out(0, q, "behz_finish: out[0] (accumulated into)");
            const u64 *d = up_in(0);
            u64 *o = flag2 ? up(a.out[0], a.out_words[0]) : ws(a.out_words[0]);
            for (size_t b = 0; b < batch; b++) fin.push_back(FinishJob{ d + b * terms * 3 * E * n, o + b * 3 * L * n, (int)terms, 0 });
            launch_behz_finish(dlevel(a.chain_idx), L, nB, jobs(fin), flag2, n, (int)batch, st_);
            down(0, o);
        } break;
        case STEP_BEHZ_FINISH_SUM: {
            need(terms >= 1, "behz_finish_sum: terms out of range");
            // the per-term canonical residues of every q limb are summed as plain integers: eval_plan.h, p.summed
            u64 widest = 0;
            for (u64 v : q) widest = std::max(widest, v);
            need((unsigned __int128)terms * widest < ((unsigned __int128)1 << 63), "behz_finish_sum: terms * q_widest reaches 2^63 (the bound of the summed finish)");
            in_is(0, batch * terms * 3 * L * n, "behz_finish_sum: in[0] [batch][terms][3][L][n]");
            in_is(1, batch * 3 * nBsk * n, "behz_finish_sum: in[1] [batch][3][nBsk][n]");
            out_is(0, batch * 3 * L * n, "behz_finish_sum: out[0] [batch][3][L][n]");
            if (!unrolled) { need(!raw, "behz_finish_sum: the generic finish has no RAW form"); canon(0, q, "behz_finish_sum: in[0]"); canon(1, bsk, "behz_finish_sum: in[1]"); }
            else need(raw, "behz_finish_sum: the unrolled finish (L == nB <= 3) takes RAW input only");
            const u64 *dq = up_in(0), *bs = up_in(1);
            u64 *o = ws(a.out_words[0]);
            for (size_t b = 0; b < batch; b++) fsum.push_back(FinishSumJob{ dq + b * terms * 3 * L * n, bs + b * 3 * nBsk * n, o + b * 3 * L * n, (int)terms, 0 });
            launch_behz_finish_sum(dlevel(a.chain_idx), L, nB, jobs(fsum), n, (int)batch, st_);
            down(0, o);
        } break;
        case STEP_KS_INNER:
        case STEP_KS_MODDOWN: {
            need(hp_.using_keyswitching, "key switching: the parameters have one prime");
            std::vector<u64> acc_mods = q;
            acc_mods.push_back(hp_.key_q[K - 1]);
            if (a.step == STEP_KS_INNER) {
                need(!raw, "ks_inner: launch_ks_inner has no RAW form");
                in_is(0, batch * (L + 1) * L * n, "ks_inner: in[0] [batch][L + 1][L][n]");
                in_is(1, (size_t)(K - 1) * 2 * K * n, "ks_inner: in[1] [K - 1][2][K][n]");
                out_is(0, batch * 2 * (L + 1) * n, "ks_inner: out[0] [batch][2][L + 1][n]");
                std::vector<u64> td_mods;                               // limb (I, J) lives modulo m_I
                for (int I = 0; I <= L; I++) for (int J = 0; J < L; J++) td_mods.push_back(acc_mods[I]);
                canon(0, td_mods, "ks_inner: in[0]");
                canon(1, hp_.key_q, "ks_inner: in[1]");
                u64 *o = ws(a.out_words[0]);
                launch_ks_inner(dkey(), L, up_in(0), up_in(1), o, n, (int)batch, st_);
                down(0, o);
                break;
            }
            need(polys == 2 || polys == 3, "ks_moddown: polys (polynomials per ciphertext slot) is 2 or 3");
            need(!raw || L <= 4, "ks_moddown: launch_ks_moddown has no RAW form above four limbs");
            need(a.n_ext >= 0 && (size_t)a.n_ext <= batch, "ks_moddown: n_ext out of range");
            need(a.n_ext == 0 || unrolled, "ks_moddown: the fused extension exists for the unrolled sizes only (L == nB <= 3)");
            in_is(0, batch * 2 * (L + 1) * n, "ks_moddown: in[0] [batch][2][L + 1][n]");
            out_is(0, batch * polys * L * n, "ks_moddown: out[0] [batch][polys][L][n]");
            if (a.n_ext) out_is(1, (size_t)a.n_ext * 2 * E * n, "ks_moddown: out[1] [n_ext][2][E][n]");
            if (!raw) canon(0, acc_mods, "ks_moddown: in[0]");
            canon_out(0, q, "ks_moddown: out[0] (added into)");
            u64 *ct = up(a.out[0], a.out_words[0]);
            u64 *ex = a.n_ext ? ws(a.out_words[1]) : nullptr;
            launch_ks_moddown(dkey(), L, up_in(0), ct, polys * L * n, n, (int)batch, st_, dlevel(a.chain_idx), ex, a.n_ext, raw);
            down(0, ct);
            if (ex) down(1, ex);
        } break;
        case STEP_MODSWITCH:
        case STEP_MODSWITCH_JOBS: {
            need(!raw, "modswitch: no RAW form");
            need(L >= 2, "modswitch: end of the modulus switching chain");
            need(polys >= 1 && polys <= 16, "modswitch: polys out of range");
            in_is(0, batch * polys * L * n, "modswitch: in[0] [batch][polys][L][n]");
            out_is(0, batch * polys * (L - 1) * n, "modswitch: out[0] [batch][polys][L - 1][n]");
            canon(0, q, "modswitch: in[0]");
            const u64 *x = up_in(0);
            u64 *o = ws(a.out_words[0]);
            if (a.step == STEP_MODSWITCH) launch_modswitch(dlevel(a.chain_idx), x, polys * L * n, (int)polys, o, n, (int)batch, st_);
            else {
                for (size_t b = 0; b < batch; b++) cj.push_back(CtJob{ x + b * polys * L * n, o + b * polys * (L - 1) * n });
                launch_modswitch_jobs(dlevel(a.chain_idx), jobs(cj), (int)polys, n, (int)batch, st_);
            }
            down(0, o);
        } break;
        case STEP_I0_FINISH: {
            need(L >= 2, "i0_finish: chain_idx is the level BEFORE the drop");
            need(terms >= 1, "i0_finish: terms out of range");
            need((unsigned __int128)(terms + 1) * q[L - 1] < ((unsigned __int128)1 << 64), "i0_finish: (terms + 1) * q_last reaches 2^64 (eval_plan.h, p.i0_fast)");
            const std::vector<u64> kept(q.begin(), q.end() - 1), last{ q[L - 1] };
            in_is(0, batch * 2 * (L - 1) * n, "i0_finish: in[0] [batch][2][L - 1][n]");
            in_is(1, batch * terms * 2 * n, "i0_finish: in[1] [batch][terms][2][n]");
            out_is(0, batch * 2 * (L - 1) * n, "i0_finish: out[0] [batch][2][L - 1][n]");
            if (!raw) { canon(0, kept, "i0_finish: in[0]"); canon(1, last, "i0_finish: in[1]"); }
            if (!store) canon_out(0, kept, "i0_finish: out[0] (accumulated into)");
            const u64 *s = up_in(0), *v = up_in(1);
            u64 *o = up(a.out[0], a.out_words[0]);
            for (size_t b = 0; b < batch; b++) ij.push_back(I0Job{ s + b * 2 * (L - 1) * n, v + b * terms * 2 * n, o + b * 2 * (L - 1) * n, (int)terms, store ? 1 : 0 });
            launch_i0_finish(dlevel(a.chain_idx), jobs(ij), n, (int)batch, st_, raw);
            down(0, o);
        } break;
        case STEP_EVAL_EPILOGUE: {
            in_is(0, batch * 2 * L * n, "eval_epilogue: in[0] [batch][2][L][n]");
            in_is(1, batch * n, "eval_epilogue: in[1] (a0) [batch][n]");
            in_is(2, batch * n, "eval_epilogue: in[2] (mask) [batch][n]");
            for (int i = 3; i <= 4; i++) if (a.in[i]) { in_is(i, batch * 2 * L * n, "eval_epilogue: addend [batch][2][L][n]"); canon(i, q, "eval_epilogue: addend"); }
            out_is(0, batch * 2 * n, "eval_epilogue: out[0] [batch][2][n]");
            canon(0, q, "eval_epilogue: in[0]");
            canon(1, tmod, "eval_epilogue: in[1] (a0 mod t)");
            canon(2, tmod, "eval_epilogue: in[2] (mask mod t)");
            if (with_key) {
                need(hp_.using_keyswitching, "eval_epilogue: the parameters have one prime");
                need(L <= 4, "eval_epilogue: the fused mod-down is a RAW form (at most four limbs)");
                in_is(5, batch * 2 * (L + 1) * n, "eval_epilogue: in[5] (RAW key-switch sums) [batch][2][L + 1][n]");
            } else need(!a.in[5], "eval_epilogue: key-switch sums given without the key flag");
            const u64 *ct = up_in(0), *a0 = up_in(1), *mk = up_in(2), *ad1 = a.in[3] ? up_in(3) : nullptr, *ad2 = a.in[4] ? up_in(4) : nullptr;
            const u64 *ks = with_key ? up_in(5) : nullptr;
            u64 *o = ws(a.out_words[0]);
            for (size_t b = 0; b < batch; b++)
                ej.push_back(EpiJob{ ct + b * 2 * L * n, ad1 ? ad1 + b * 2 * L * n : nullptr, ad2 ? ad2 + b * 2 * L * n : nullptr, a0 + b * n, mk + b * n, o + b * 2 * n,
                                     ks ? ks + b * 2 * (L + 1) * n : nullptr });
            launch_eval_epilogue(dlevel(0), a.chain_idx, jobs(ej), (size_t)L * n, hp_.irrelevant_bit_count, n, (int)batch, st_, with_key ? dkey() : nullptr);
            down(0, o);
        } break;
        case STEP_ADD_MANY:
        case STEP_SUM_JOBS: {
            need(terms >= 1 && terms <= 4096, "add_many / sum_jobs: terms out of range");
            need(polys >= 1 && polys <= 16, "add_many / sum_jobs: polys out of range");
            in_is(0, batch * terms * polys * L * n, "add_many / sum_jobs: in[0] [batch][terms][polys][L][n]");
            out_is(0, batch * polys * L * n, "add_many / sum_jobs: out[0] [batch][polys][L][n]");
            canon(0, q, "add_many / sum_jobs: in[0]");
            const u64 *x = up_in(0);
            if (a.step == STEP_ADD_MANY) {
                canon_out(0, q, "add_many: out[0] (added into)");
                u64 *o = up(a.out[0], a.out_words[0]);
                launch_add_many(dlevel(a.chain_idx), o, polys * L * n, x, (int)terms, (int)polys, n, (int)batch, st_);
                down(0, o);
            } else {
                need(n % 2 == 0, "sum_jobs: two coefficients per lane");
                u64 *o = ws(a.out_words[0]);
                for (size_t b = 0; b < batch; b++) sj.push_back(SumJob{ x + b * terms * polys * L * n, o + b * polys * L * n, (int)terms, 0 });
                launch_sum_jobs(dlevel(a.chain_idx), L, jobs(sj), (int)polys, n, (int)batch, st_);
                down(0, o);
            }
        } break;
        case STEP_ADD_PLAIN: {
            in_is(0, batch * n, "add_plain: in[0] [batch][n]");
            out_is(0, batch * L * n, "add_plain: out[0] [batch][L][n]");
            canon(0, tmod, "add_plain: in[0] (mod t)");
            canon_out(0, q, "add_plain: out[0] (added into)");
            const u64 *pt = up_in(0);
            u64 *o = up(a.out[0], a.out_words[0]);
            for (size_t b = 0; b < batch; b++) pj.push_back(PlainJob{ o + b * L * n, pt + b * n });
            launch_add_plain(dlevel(a.chain_idx), jobs(pj), n, (int)batch, st_);
            down(0, o);
        } break;
        case STEP_DYADIC_PLAIN: {
            need(polys >= 1 && polys <= 16, "dyadic_plain: polys out of range");
            in_is(0, batch * polys * L * n, "dyadic_plain: in[0] [batch][polys][L][n]");
            in_is(1, batch * L * n, "dyadic_plain: in[1] [batch][L][n]");
            out_is(0, batch * polys * L * n, "dyadic_plain: out[0] [batch][polys][L][n]");
            canon(0, q, "dyadic_plain: in[0]");
            canon(1, q, "dyadic_plain: in[1]");
            u64 *o = ws(a.out_words[0]);
            launch_dyadic_plain(dlevel(a.chain_idx), up_in(0), up_in(1), o, (int)polys, n, (int)batch, (size_t)L * n, st_);
            down(0, o);
        } break;
        case STEP_LIFT: {
            in_is(0, batch * n, "lift: in[0] [batch][n]");
            out_is(0, batch * L * n, "lift: out[0] [batch][L][n]");
            canon(0, tmod, "lift: in[0] (mod t)");
            const unsigned char *nl = nullptr;
            if (a.in[1]) {                                              // one word per plaintext, non-zero: the monomial shortcut (no lift)
                in_is(1, batch, "lift: in[1] [batch]");
                flags8.resize((batch + 7) / 8 * 8, 0);
                for (size_t b = 0; b < batch; b++) flags8[b] = a.in[1][b] != 0;
                nl = reinterpret_cast<const unsigned char *>(up(reinterpret_cast<const u64 *>(flags8.data()), flags8.size() / 8));
            }
            u64 *o = ws(a.out_words[0]);
            launch_lift(dlevel(a.chain_idx), up_in(0), o, n, (int)batch, nl, st_);
            down(0, o);
        } break;
        default: refuse("unknown step");
        }
        sync();
    });
}

} // namespace apsu_he
