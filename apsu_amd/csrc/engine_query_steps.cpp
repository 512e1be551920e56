// One querier-side or decryption kernel at a time on caller-chosen words (Engine::debug_run_step from STEP_SEED_EXPAND on;
// include/apsu_he.h).  As engine_steps.cpp, engine_db_steps.cpp and engine_ntt_steps.cpp do for their families: a step copies host
// arrays up, calls THE launcher engine_query.cpp calls -- launch_seed_expand, launch_decrypt_round(_budget), launch_plain_powers, the
// two samplers, launch_small_lift, launch_enc_finish, launch_rlk_finish, launch_flag_monomial (launch_ew.h) -- with the context's own
// DevLevel / DevKey blocks and slot map, synchronises and copies back.  Signed bytes (the small polynomials) and 32-bit words travel as
// one 64-bit word per entry, a signed byte sign-extended, and are narrowed here.  out[0] is copied up first everywhere, so a word the
// kernel does not write comes back as it went.  Whatever a launcher's contract does not admit is refused before anything is launched.
// For the tests; nothing on the query path calls it.
#include "engine_impl.h"
#include "query_side.h"

#include <functional>
#include <list>
#include <string>

namespace apsu_he {

namespace {

[[noreturn]] void refuse(const std::string &why) { throw std::invalid_argument("debug_run_step: " + why); }
void need(bool ok, const char *why) { if (!ok) refuse(why); }

void canonical(const u64 *x, size_t words, u64 m, const char *what)
{
    u64 bad = 0;
    for (size_t k = 0; k < words; k++) bad |= (u64)(x[k] >= m);
    if (bad) refuse(std::string(what) + " holds a word that is not a canonical residue of its modulus");
}

void fits_int8(const u64 *x, size_t words, const char *what)
{
    u64 bad = 0;
    for (size_t k = 0; k < words; k++) bad |= (u64)((int64_t)x[k] < -128 || (int64_t)x[k] > 127);
    if (bad) refuse(std::string(what) + " holds a word that is not a sign-extended signed byte");
}

} // namespace

void Engine::debug_run_query_step(const StepArgs &a)
{
    const size_t n = hp_.n;
    const int K = hp_.K;
    const u64 t = hp_.t;
    const size_t batch = a.batch > 0 ? (size_t)a.batch : 0, terms = a.terms > 0 ? (size_t)a.terms : 0, polys = a.polys > 0 ? (size_t)a.polys : 0;
    auto in_is = [&](int i, size_t words, const char *what) { if (!a.in[i] || a.in_words[i] != words) refuse(std::string(what) + ": wrong size"); };
    auto out_is = [&](int i, size_t words, const char *what) { if (!a.out[i] || a.out_words[i] != words) refuse(std::string(what) + ": wrong size"); };
    need(a.step >= STEP_SEED_EXPAND && a.step < STEP_MAC_INFO, "unknown step");
    need(batch >= 1 && batch <= 64, "batch out of range (1 .. 64)");

    // ---- everything a launcher's contract does not admit is refused here, in front of the arena: nothing below can refuse
    int L = 0;                                                       // limbs of the step's level
    size_t S = 0, limbs = 0;
    const bool budget = a.flags & STEP_ACCUMULATE, cbd = a.flags & STEP_KEY;
    switch (a.step) {
    case STEP_SEED_EXPAND: {
        // chain_idx (-1 or K - 1: the key level), terms = the list cap; in[0] seeds [batch][8], in[1] thresholds [L] (in place of SEAL's
        // max_multiple) -> out[0] [batch][L][n] in/out, out[1] the lists' counters as k_seed_fix left them [batch], then the overflow word
        const bool key_level = a.chain_idx < 0 || a.chain_idx == K - 1;
        if (!key_level) check_level(a.chain_idx);
        L = key_level ? K : a.chain_idx + 1;
        need(L <= DMAXL, "seed_expand: more limbs than the device tables hold");
        need(terms >= 1 && terms <= SEED_REJ_CAP, "seed_expand: the list cap (terms) is outside 1 .. 8192");
        in_is(0, batch * 8, "seed_expand: in[0] seeds [batch][8]");
        in_is(1, (size_t)L, "seed_expand: in[1] thresholds [L]");
        // k_seed_fix redraws until a word falls below the threshold: a small one is a hang.  Every real one exceeds 2^63 (q < 2^62).
        for (int j = 0; j < L; j++) need(a.in[1][j] >> 62, "seed_expand: a threshold below 2^62 (the redraw loop ends only with a draw below it)");
        out_is(0, batch * (size_t)L * n, "seed_expand: out[0] [batch][L][n]");
        out_is(1, batch + 1, "seed_expand: out[1] counters [batch], overflow");
    } break;
    case STEP_DECRYPT_ROUND: {
        // in[0] ct [batch][2][n] (c0 is read), in[1] v [batch][n], in[2] q0, t -> out[0] [batch][n]; ACCUMULATE: launch_decrypt_round_budget,
        // out[1] worst [batch]
        in_is(0, batch * 2 * n, "decrypt_round: in[0] ct [batch][2][n]");
        in_is(1, batch * n, "decrypt_round: in[1] v [batch][n]");
        in_is(2, 2, "decrypt_round: in[2] q0, t");
        const u64 q0 = a.in[2][0], tt = a.in[2][1];
        need(!(q0 >> 62) && !(tt >> 61) && tt >= 2 && tt < q0, "decrypt_round: needs 2 <= t < q0 < 2^62 and t < 2^61");
        for (size_t b = 0; b < batch; b++) canonical(a.in[0] + b * 2 * n, n, q0, "decrypt_round: in[0] (a c0)");
        canonical(a.in[1], batch * n, q0, "decrypt_round: in[1]");
        out_is(0, batch * n, "decrypt_round: out[0] [batch][n]");
        if (budget) out_is(1, batch, "decrypt_round: out[1] worst [batch]");
    } break;
    case STEP_PLAIN_POWERS: {
        // in[0] values [batch][n] (any words: the flag is the subject), in[1] exponents [S] -> out[0] [batch * S][n] in/out, out[1] the flag word
        need(hp_.batching, "plain_powers: plain_modulus does not support batching (no slot map)");
        S = a.in_words[1];
        need(a.in[1] && S >= 1 && S <= 64, "plain_powers: in[1] exponents: 1 .. 64 entries");
        for (size_t s = 0; s < S; s++) need(!(a.in[1][s] >> 32), "plain_powers: an exponent does not fit 32 bits");
        in_is(0, batch * n, "plain_powers: in[0] values [batch][n]");
        out_is(0, batch * S * n, "plain_powers: out[0] [batch * S][n]");
        out_is(1, 1, "plain_powers: out[1] the flag word");
    } break;
    case STEP_SAMPLE_SMALL: {
        // in[0] seed [8] -> out[0] [n] the secret's coefficients (batch 1, e0 0); KEY: the noise of objects e0 .. e0 + batch - 1, [batch][n]
        in_is(0, 8, "sample_small: in[0] seed [8]");
        need(n % 8 == 0, "sample_small: n is no multiple of 8");
        if (cbd) need(a.e0 >= 0 && (u64)a.e0 + batch <= QS_MAX_OBJECTS, "sample_small: objects (e0 .. e0 + batch) outside the seed's range");
        else need(batch == 1 && a.e0 == 0, "sample_small: the secret is one polynomial (batch 1, e0 0)");
        out_is(0, batch * n, "sample_small: out[0] [batch][n]");
    } break;
    case STEP_SMALL_LIFT: {
        // polys = limbs (1 .. K); in[0] small [batch][n] signed bytes -> out[0] [batch][limbs][n]
        limbs = polys;
        need(limbs >= 1 && limbs <= (size_t)K && K <= DMAXL + 1, "small_lift: limbs (polys) outside 1 .. K");
        in_is(0, batch * n, "small_lift: in[0] small [batch][n]");
        fits_int8(a.in[0], batch * n, "small_lift: in[0]");
        out_is(0, batch * limbs * n, "small_lift: out[0] [batch][limbs][n]");
    } break;
    case STEP_ENC_FINISH: {
        // in[0] pt [batch][n] mod t, in[1] v [batch][L][n], in[2] e [batch][n] signed bytes -> out[0] cts [batch][2][L][n] in/out (c0 written)
        check_level(a.chain_idx);
        L = a.chain_idx + 1;
        in_is(0, batch * n, "enc_finish: in[0] pt [batch][n]");
        in_is(1, batch * (size_t)L * n, "enc_finish: in[1] v [batch][L][n]");
        in_is(2, batch * n, "enc_finish: in[2] e [batch][n]");
        out_is(0, batch * 2 * (size_t)L * n, "enc_finish: out[0] cts [batch][2][L][n]");
        canonical(a.in[0], batch * n, t, "enc_finish: in[0]");
        for (size_t r = 0; r < batch * (size_t)L; r++) canonical(a.in[1] + r * n, n, hp_.key_q[r % (size_t)L], "enc_finish: in[1]");
        fits_int8(a.in[2], batch * n, "enc_finish: in[2]");
    } break;
    case STEP_RLK_FINISH: {
        // in[0] s [K][n], in[1] e [K - 1][K][n] -> out[0] ksk [K - 1][2][K][n] in/out: the a halves [i][1] are read, the c0 halves written
        need(K >= 2 && K <= DMAXL + 1, "rlk_finish: a context with one prime has no relinearisation keys");
        need(batch == 1, "rlk_finish: one key set per launch (batch 1)");
        in_is(0, (size_t)K * n, "rlk_finish: in[0] s [K][n]");
        in_is(1, (size_t)(K - 1) * K * n, "rlk_finish: in[1] e [K - 1][K][n]");
        out_is(0, (size_t)(K - 1) * 2 * K * n, "rlk_finish: out[0] ksk [K - 1][2][K][n]");
        for (int j = 0; j < K; j++) canonical(a.in[0] + (size_t)j * n, n, hp_.key_q[j], "rlk_finish: in[0]");
        for (int i = 0; i < K - 1; i++)
            for (int j = 0; j < K; j++) {
                canonical(a.in[1] + ((size_t)i * K + j) * n, n, hp_.key_q[j], "rlk_finish: in[1]");
                canonical(a.out[0] + (((size_t)i * 2 + 1) * K + j) * n, n, hp_.key_q[j], "rlk_finish: out[0] (an a half)");
            }
    } break;
    case STEP_FLAG_MONOMIAL: {
        // in[0] pt [batch][n] (any words: only tested for zero) -> out[0] [batch], 1 where exactly one word is non-zero
        in_is(0, batch * n, "flag_monomial: in[0] pt [batch][n]");
        out_is(0, batch, "flag_monomial: out[0] [batch]");
    } break;
    default: refuse("unknown step");
    }

    // host copies of the narrowed arrays and the widening of what comes back: both outlive the queued copies (the call ends with a sync)
    std::list<std::vector<u32>> keep32;
    std::list<std::vector<signed char>> keep8;
    std::vector<SeedJob> sj;
    std::vector<std::function<void()>> after;

    WITH_ARENA({
        keep32.clear(); keep8.clear(); sj.clear(); after.clear();      // a retry with a larger arena starts over
        auto up = [&](const u64 *src, size_t words) {
            u64 *d = ws(words + 1);
            if (words) HIP_CHECK(hipMemcpyAsync(d, src, words * sizeof(u64), hipMemcpyHostToDevice, st_));
            return d;
        };
        auto up32 = [&](const u64 *src, size_t words) {
            keep32.emplace_back(words);
            std::vector<u32> &h = keep32.back();
            for (size_t i = 0; i < words; i++) h[i] = (u32)src[i];
            u32 *d = ws_as<u32>(words, 1);
            HIP_CHECK(hipMemcpyAsync(d, h.data(), words * sizeof(u32), hipMemcpyHostToDevice, st_));
            return d;
        };
        auto up8 = [&](const u64 *src, size_t words) {
            keep8.emplace_back(words);
            std::vector<signed char> &h = keep8.back();
            for (size_t i = 0; i < words; i++) h[i] = (signed char)(int64_t)src[i];
            signed char *d = ws_as<signed char>(words, 1);
            HIP_CHECK(hipMemcpyAsync(d, h.data(), words, hipMemcpyHostToDevice, st_));
            return d;
        };
        auto down = [&](u64 *dst, const u64 *src, size_t words) { if (words) HIP_CHECK(hipMemcpyAsync(dst, src, words * sizeof(u64), hipMemcpyDeviceToHost, st_)); };
        auto down8 = [&](u64 *dst, const void *src, size_t words, bool is_signed) {
            keep8.emplace_back(words);
            std::vector<signed char> *h = &keep8.back();
            HIP_CHECK(hipMemcpyAsync(h->data(), src, words, hipMemcpyDeviceToHost, st_));
            after.push_back([=] { for (size_t i = 0; i < words; i++) dst[i] = is_signed ? (u64)(int64_t)(*h)[i] : (u64)(unsigned char)(*h)[i]; });
        };

        switch (a.step) {
        case STEP_SEED_EXPAND: {
            const DevLevel *lv = seed_level(L);
            u64 *o = up(a.out[0], a.out_words[0]);
            for (size_t b = 0; b < batch; b++) {
                SeedJob j;
                for (int k = 0; k < 8; k++) j.seed.w[k] = a.in[0][b * 8 + k];
                j.dst = o + b * (size_t)L * n;
                sj.push_back(j);
            }
            SeedJob *dj = ws_as<SeedJob>(batch, 1);
            HIP_CHECK(hipMemcpyAsync(dj, sj.data(), batch * sizeof(SeedJob), hipMemcpyHostToDevice, st_));
            const size_t rej_words = batch * (1 + (size_t)SEED_REJ_CAP) + 1;       // fresh lists, then the overflow word: the engine's layout
            u32 *rej = ws_as<u32>(rej_words, 1);
            HIP_CHECK(hipMemsetAsync(rej, 0, rej_words * sizeof(u32), st_));
            int *overflow = reinterpret_cast<int *>(rej + batch * (1 + (size_t)SEED_REJ_CAP));
            launch_seed_expand(dj, (int)batch, lv, L, up(a.in[1], (size_t)L), n, rej, (u32)terms, overflow, st_);
            down(a.out[0], o, a.out_words[0]);
            keep32.emplace_back(batch + 1);
            std::vector<u32> *h = &keep32.back();
            for (size_t b = 0; b <= batch; b++)
                HIP_CHECK(hipMemcpyAsync(h->data() + b, rej + b * (1 + (size_t)SEED_REJ_CAP), sizeof(u32), hipMemcpyDeviceToHost, st_));
            u64 *dst = a.out[1];
            after.push_back([=] { for (size_t b = 0; b <= batch; b++) dst[b] = (*h)[b]; });
        } break;
        case STEP_DECRYPT_ROUND: {
            const u64 q0 = a.in[2][0], tt = a.in[2][1];
            const u64 *ct = up(a.in[0], a.in_words[0]), *v = up(a.in[1], a.in_words[1]);
            u64 *o = up(a.out[0], a.out_words[0]);
            if (budget) {
                u64 *worst = ws(batch);
                HIP_CHECK(hipMemsetAsync(worst, 0, batch * sizeof(u64), st_));
                launch_decrypt_round_budget(ct, 2 * n, v, q0, tt, o, n, (int)batch, worst, st_);
                down(a.out[1], worst, batch);
            } else
                launch_decrypt_round(ct, 2 * n, v, q0, tt, o, n, (int)batch, st_);
            down(a.out[0], o, a.out_words[0]);
        } break;
        case STEP_PLAIN_POWERS: {
            const u64 *vals = up(a.in[0], a.in_words[0]);
            const u32 *exps = up32(a.in[1], S);
            u64 *o = up(a.out[0], a.out_words[0]);
            u64 *flags = ws(1);
            HIP_CHECK(hipMemsetAsync(flags, 0, sizeof(u64), st_));
            launch_plain_powers(vals, reinterpret_cast<const uint32_t *>(d_slot_map_.p()), exps, (int)S, make_mod(t), o, n, (int)batch,
                                reinterpret_cast<u32 *>(flags), st_);
            down(a.out[0], o, a.out_words[0]);
            down(a.out[1], flags, 1);
        } break;
        case STEP_SAMPLE_SMALL: {
            Blake2xbSeed sd;
            for (int k = 0; k < 8; k++) sd.w[k] = a.in[0][k];
            signed char *small = reinterpret_cast<signed char *>(ws(batch * n / 8));
            if (cbd) launch_sample_cbd(sd, (u64)a.e0, small, n, (int)batch, st_);
            else launch_sample_ternary(sd, small, n, st_);
            down8(a.out[0], small, batch * n, true);
        } break;
        case STEP_SMALL_LIFT: {
            const signed char *small = up8(a.in[0], batch * n);
            u64 *o = up(a.out[0], a.out_words[0]);
            launch_small_lift(dkey(), small, o, (int)limbs, n, (int)batch, st_);
            down(a.out[0], o, a.out_words[0]);
        } break;
        case STEP_ENC_FINISH: {
            const u64 *pt = up(a.in[0], a.in_words[0]), *v = up(a.in[1], a.in_words[1]);
            const signed char *e = up8(a.in[2], batch * n);
            u64 *cts = up(a.out[0], a.out_words[0]);
            launch_enc_finish(dlevel(a.chain_idx), pt, v, e, cts, n, (int)batch, st_);
            down(a.out[0], cts, a.out_words[0]);
        } break;
        case STEP_RLK_FINISH: {
            const u64 *s = up(a.in[0], a.in_words[0]), *e = up(a.in[1], a.in_words[1]);
            u64 *ksk = up(a.out[0], a.out_words[0]);
            launch_rlk_finish(dkey(), K, s, e, ksk, n, st_);
            down(a.out[0], ksk, a.out_words[0]);
        } break;
        default: {                                                     // STEP_FLAG_MONOMIAL
            const u64 *pt = up(a.in[0], a.in_words[0]);
            unsigned char *flag = ws_as<unsigned char>(batch, 1);
            HIP_CHECK(hipMemsetAsync(flag, 0xff, batch, st_));
            launch_flag_monomial(pt, n, (int)batch, flag, st_);
            down8(a.out[0], flag, batch, false);
        } break;
        }
        sync();
        for (auto &f : after) f();
    });
}

} // namespace apsu_he
