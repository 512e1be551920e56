// One transform launch at a time on caller-chosen words (Engine::debug_run_step from STEP_NTT_INFO on; include/apsu_he.h).
// As engine_steps.cpp and engine_db_steps.cpp do for the kernels between the transforms: a step copies host arrays up, calls THE
// launcher the engine calls -- launch_ntt, launch_ntt_gather, launch_intt_tensor (launch_ntt.h) -- with the context's own tabs(), its
// own ntt_latency_limbs setting and a limb-to-modulus map given by the caller, so ntt_form, the form tables and the split path at
// n = 32768 are part of what runs; "every modulus of the launch is narrow" is computed here the way the engine's callers state it
// (ntt_is_narrow at the ring's logn, as dev_consts.cpp computes data_primes_narrow; at n = 32768 the tables' own `narrow` is for the 14
// stages a workgroup runs, and ntt_form does not look at the statement there).  Whatever a launcher's input contract (launch_ntt.h) does not admit is refused before anything
// is launched.  For the tests; nothing on the query path calls it.
#include "engine_impl.h"

#include <string>

namespace apsu_he {

namespace {

[[noreturn]] void refuse(const std::string &why) { throw std::invalid_argument("debug_run_step: " + why); }
void need(bool ok, const char *why) { if (!ok) refuse(why); }

constexpr size_t NTT_STEP_MAX_LIMBS = 4096;                          // of one launch: far above what a test needs, keeps limbs * n small

void canonical_limb(const u64 *x, size_t n, u64 m, const char *what)
{
    u64 bad = 0;
    for (size_t k = 0; k < n; k++) bad |= (u64)(x[k] >= m);
    if (bad) refuse(std::string(what) + " holds a word that is not a canonical residue of its limb's modulus");
}

} // namespace

void Engine::debug_run_ntt_step(const StepArgs &a)
{
    const size_t n = hp_.n;
    const int logn = hp_.logn, nmod = (int)hp_.ntt.size();
    auto modulus = [&](int id) { return hp_.ntt[(size_t)id].mod.value; };
    auto in_is = [&](int i, size_t words, const char *what) { if (!a.in[i] || a.in_words[i] != words) refuse(std::string(what) + ": wrong size"); };
    auto out_is = [&](int i, size_t words, const char *what) { if (!a.out[i] || a.out_words[i] != words) refuse(std::string(what) + ": wrong size"); };

    if (a.step == STEP_NTT_INFO) {
        // logn, K, the number of auxiliary primes, batching, then the modulus of every modulus id (0 .. K-1 key primes, K + i aux_primes[i],
        // plain_id() where batching is on)
        need(a.out[0] && a.out_words[0] >= 4 + (size_t)nmod, "ntt_info: out[0] too small");
        u64 *o = a.out[0];
        *o++ = (u64)logn; *o++ = (u64)hp_.K; *o++ = (u64)hp_.aux_primes.size(); *o++ = hp_.batching ? 1 : 0;
        for (int id = 0; id < nmod; id++) *o++ = modulus(id);
        return;
    }

    // the map as the launcher reads it: in[map_at] [period], entry = modulus id, NTT_MAP_RAW on top where `raw_ok`
    std::vector<int> map;
    bool narrow = true;
    auto read_map = [&](int map_at, bool raw_ok, const char *what) {
        const size_t period = a.in_words[map_at];
        if (!a.in[map_at] || period < 1 || period > NTT_STEP_MAX_LIMBS) refuse(std::string(what) + ": the map has 1 .. 4096 entries");
        map.resize(period);
        for (size_t i = 0; i < period; i++) {
            const u64 v = a.in[map_at][i];
            if ((v & ~(u64)NTT_MAP_RAW) >= (u64)nmod) refuse(std::string(what) + ": a map entry names a modulus id out of range");
            if ((v & NTT_MAP_RAW) && !raw_ok) refuse(std::string(what) + ": NTT_MAP_RAW in the map of a forward transform");
            map[i] = (int)v;
            narrow = narrow && ntt_is_narrow(modulus((int)(v & NTT_MAP_MASK)), logn);
        }
    };
    auto map_mod = [&](size_t g) { return modulus(map[g % map.size()] & NTT_MAP_MASK); };

    // ---- everything a launcher's contract does not admit is refused here, in front of the arena: nothing below can refuse
    size_t count = 0, nsrc = 0, njobs = 0, limbs = 0, stride = 0, dgap = 0, n_plain = 0, n_tensor = 0;
    bool inverse = false, nored = false;
    switch (a.step) {
    case STEP_NTT: {
        // in[0] [count][n] canonical, in[1] map [period]; STEP_INVERSE: the inverse transform (the map may carry NTT_MAP_RAW) -> out[0] [count][n]
        inverse = a.flags & STEP_INVERSE;
        need(a.in[0] && a.in_words[0] >= n && a.in_words[0] % n == 0 && a.in_words[0] / n <= NTT_STEP_MAX_LIMBS, "ntt: in[0] [count][n], 1 .. 4096 limbs");
        count = a.in_words[0] / n;
        out_is(0, count * n, "ntt: out[0] [count][n]");
        read_map(1, inverse, "ntt");
        for (size_t g = 0; g < count; g++) canonical_limb(a.in[0] + g * n, n, map_mod(g), "ntt: in[0]");
    } break;
    case STEP_NTT_GATHER: {
        // in[0] sources [nsrc][n], in[1] the source of every output limb [count], in[2] map [period], in[3] max_src (one word; STEP_NORED:
        // no reduction on load, every source word below it) -> out[0] [count][n]
        nored = a.flags & STEP_NORED;
        need(a.in[0] && a.in_words[0] >= n && a.in_words[0] % n == 0, "ntt_gather: in[0] sources [nsrc][n]");
        nsrc = a.in_words[0] / n;
        count = a.in_words[1];
        need(a.in[1] && count >= 1 && count <= NTT_STEP_MAX_LIMBS, "ntt_gather: in[1] source index per output limb, 1 .. 4096 limbs");
        out_is(0, count * n, "ntt_gather: out[0] [count][n]");
        read_map(2, false, "ntt_gather");
        for (size_t g = 0; g < count; g++) need(a.in[1][g] < nsrc, "ntt_gather: a source index is not below the number of sources");
        if (nored) {
            in_is(3, 1, "ntt_gather: in[3] max_src (one word)");
            const u64 max_src = a.in[3][0];
            need(logn < SPLIT_LOGN, "ntt_gather: no unreduced gather at n = 32768 (the engine never asks for it)");
            for (int v : map) need(ntt_gather_nored_ok(modulus(v), max_src, logn), "ntt_gather: a target modulus fails ntt_gather_nored_ok for max_src");
            u64 bad = 0;
            for (size_t i = 0; i < a.in_words[0]; i++) bad |= (u64)(a.in[0][i] >= max_src);
            need(!bad, "ntt_gather: a source word is not below max_src");
        }
    } break;
    case STEP_INTT_TENSOR: {
        // batch = njobs, terms = limbs, polys = stride (limbs between the two polynomials of an operand, >= limbs; 0: limbs), e0 = dgap
        // (limbs between the outputs of two jobs, >= 3 limbs; 0: 3 limbs); in[0] a [njobs][2][stride][n], in[1] b the same, in[2] plain
        // [n_plain][n] or null, in[3] map [period] over the launch's logical limbs (job, poly of 3, limb), then the plain ones ->
        // out[0] [njobs][dgap][n] in/out: job j's [3][limbs][n] at its start, the words behind come back as they went; out[1] [n_plain][n]
        njobs = a.batch > 0 ? (size_t)a.batch : 0;
        limbs = a.terms > 0 ? (size_t)a.terms : 0;
        stride = a.polys > 0 ? (size_t)a.polys : limbs;
        dgap = a.e0 > 0 ? (size_t)a.e0 : 3 * limbs;
        n_plain = a.in[2] ? a.in_words[2] / n : 0;
        need(logn < SPLIT_LOGN, "intt_tensor: launch_intt_tensor has no form at n = 32768");
        need(njobs <= 64 && limbs <= 64 && stride >= limbs && stride <= 64 && dgap >= 3 * limbs && dgap <= 256 && (njobs == 0) == (limbs == 0),
             "intt_tensor: njobs (batch), limbs (terms), stride (polys) or dgap (e0) out of range");
        n_tensor = njobs * 3 * limbs;
        need(n_tensor + n_plain >= 1 && n_plain <= NTT_STEP_MAX_LIMBS, "intt_tensor: an empty launch, or too many plain limbs");
        if (njobs) { in_is(0, njobs * 2 * stride * n, "intt_tensor: in[0] a [njobs][2][stride][n]"); in_is(1, njobs * 2 * stride * n, "intt_tensor: in[1] b [njobs][2][stride][n]"); }
        if (a.in[2]) need(a.in_words[2] == n_plain * n && n_plain >= 1, "intt_tensor: in[2] plain [n_plain][n]");
        if (njobs) out_is(0, njobs * dgap * n, "intt_tensor: out[0] [njobs][dgap][n]");
        if (n_plain) out_is(1, n_plain * n, "intt_tensor: out[1] [n_plain][n]");
        read_map(3, true, "intt_tensor");
        for (size_t jb = 0; jb < njobs; jb++)
            for (size_t e = 0; e < limbs; e++) {
                const size_t g0 = jb * 3 * limbs + e;
                const u64 m = map_mod(g0);
                need(map_mod(g0 + limbs) == m && map_mod(g0 + 2 * limbs) == m, "intt_tensor: the three outputs of one operand limb name different moduli");
                for (size_t p = 0; p < 2; p++) {
                    canonical_limb(a.in[0] + ((jb * 2 + p) * stride + e) * n, n, m, "intt_tensor: in[0]");
                    canonical_limb(a.in[1] + ((jb * 2 + p) * stride + e) * n, n, m, "intt_tensor: in[1]");
                }
            }
        for (size_t g = 0; g < n_plain; g++) canonical_limb(a.in[2] + g * n, n, map_mod(n_tensor + g), "intt_tensor: in[2]");
    } break;
    default: refuse("unknown step");
    }

    std::vector<const u64 *> srcp;
    std::vector<TensorJob> tj;

    WITH_ARENA({
        srcp.clear(); tj.clear();                                     // a retry with a larger arena starts over
        auto up = [&](const u64 *src, size_t words) {
            u64 *d = ws(words + 1);
            if (words) HIP_CHECK(hipMemcpyAsync(d, src, words * sizeof(u64), hipMemcpyHostToDevice, st_));
            return d;
        };
        auto up_map = [&]() {
            int *d = ws_as<int>(map.size(), 1);
            HIP_CHECK(hipMemcpyAsync(d, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice, st_));
            return static_cast<const int *>(d);
        };
        auto down = [&](u64 *dst, const u64 *src, size_t words) { if (words) HIP_CHECK(hipMemcpyAsync(dst, src, words * sizeof(u64), hipMemcpyDeviceToHost, st_)); };

        if (a.step == STEP_NTT) {
            u64 *d = up(a.in[0], a.in_words[0]);
            launch_ntt(logn, inverse, d, count, tabs(), up_map(), (int)map.size(), st_, sw_.ntt_latency_limbs, narrow);
            down(a.out[0], d, count * n);
        } else if (a.step == STEP_NTT_GATHER) {
            const u64 *s = up(a.in[0], a.in_words[0]);
            for (size_t g = 0; g < count; g++) srcp.push_back(s + (size_t)a.in[1][g] * n);
            const u64 **dp = ws_as<const u64 *>(count, 1);
            HIP_CHECK(hipMemcpyAsync(dp, srcp.data(), count * sizeof(const u64 *), hipMemcpyHostToDevice, st_));
            u64 *d = ws(count * n);
            launch_ntt_gather(logn, dp, d, count, tabs(), up_map(), (int)map.size(), st_, nored, sw_.ntt_latency_limbs, narrow);
            down(a.out[0], d, count * n);
        } else {
            const u64 *x = njobs ? up(a.in[0], a.in_words[0]) : nullptr, *y = njobs ? up(a.in[1], a.in_words[1]) : nullptr;
            u64 *pl = n_plain ? up(a.in[2], a.in_words[2]) : nullptr, *o = njobs ? up(a.out[0], a.out_words[0]) : ws(1);
            for (size_t jb = 0; jb < njobs; jb++) tj.push_back(TensorJob{ x + jb * 2 * stride * n, y + jb * 2 * stride * n, o + jb * dgap * n });
            TensorJob *dj = ws_as<TensorJob>(njobs, 1);
            if (njobs) HIP_CHECK(hipMemcpyAsync(dj, tj.data(), njobs * sizeof(TensorJob), hipMemcpyHostToDevice, st_));
            launch_intt_tensor(logn, dj, (int)njobs, (int)limbs, stride * n, pl, n_plain, tabs(), up_map(), (int)map.size(), st_, sw_.ntt_latency_limbs);
            if (njobs) down(a.out[0], o, njobs * dgap * n);
            down(a.out[1], pl, n_plain * n);
        }
        sync();
    });
}

} // namespace apsu_he
