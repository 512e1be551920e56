// The launchers that no other family's steps reach, one at a time on caller-chosen words (Engine::debug_run_step from STEP_ADD on;
// include/apsu_he.h): launch_add, launch_clear_bits, launch_copy_jobs, launch_copy_sources, launch_fill_random, launch_fill_blake2xb
// (launch_ew.h), launch_scatter_slots, launch_gather_slots, launch_algebraize and launch_pack_blocks (launch_db.h).  As the other
// engine_*_steps.cpp do: a step copies host arrays up, calls THE launcher the engine calls -- with the context's own level block where
// the launcher takes one, and the context's slot map where the caller gives none -- synchronises and copies back.  Every out[] is copied
// up first, so a word the kernel does not write comes back as it went.  Whatever a launcher's contract does not admit is refused before
// anything is launched.  For the tests; nothing on the query path calls it.
#include "engine_impl.h"
#include "blake2x.h"

#include <string>

namespace apsu_he {

namespace {

[[noreturn]] void refuse(const std::string &why) { throw std::invalid_argument("debug_run_step: " + why); }
void need(bool ok, const char *why) { if (!ok) refuse(why); }

constexpr size_t WORDS_MAX = (size_t)1 << 26;                          // far above every test's arrays

} // namespace

void Engine::debug_run_misc_step(const StepArgs &a)
{
    need(a.step >= STEP_ADD && a.step <= STEP_PACK_BLOCKS, "unknown step");
    const size_t n = hp_.n;
    const size_t terms = a.terms > 0 ? (size_t)a.terms : 0, polys = a.polys > 0 ? (size_t)a.polys : 0, batch = a.batch > 0 ? (size_t)a.batch : 0;
    const size_t e0 = a.e0 > 0 ? (size_t)a.e0 : 0;
    auto in_is = [&](int i, size_t words, const char *what) { if (!a.in[i] || a.in_words[i] != words) refuse(std::string(what) + ": wrong size"); };
    auto out_is = [&](int i, size_t words, const char *what) { if (!a.out[i] || a.out_words[i] != words) refuse(std::string(what) + ": wrong size"); };
    for (int i = 0; i < 6; i++) need(!a.in[i] || a.in_words[i] <= WORDS_MAX, "an input array is too large");
    for (int i = 0; i < 2; i++) need(!a.out[i] || a.out_words[i] <= WORDS_MAX, "an output array is too large");

    // ---- the refusals, all in front of the arena: nothing below can refuse
    int L = 0;
    size_t words = 0, count = 0;
    std::vector<u32> map32;
    Blake2xbSeed seed{};
    switch (a.step) {
    case STEP_ADD: {
        // chain_idx = the level; in[0] x [batch][polys][L][n] added into out[0] acc [batch][polys][L][n]; both canonical
        check_level(a.chain_idx);
        L = a.chain_idx + 1;
        const LevelConstants &h = hlevel(a.chain_idx);
        need(batch >= 1 && batch <= 64 && polys >= 1 && polys <= 8, "add: batch (1 .. 64) or polys (1 .. 8) out of range");
        words = batch * polys * (size_t)L * n;
        in_is(0, words, "add: in[0] x [batch][polys][L][n]");
        out_is(0, words, "add: out[0] acc [batch][polys][L][n]");
        for (size_t r = 0; r < batch * polys * (size_t)L; r++) {
            const u64 q = h.q[r % (size_t)L];
            u64 bad = 0;
            for (size_t k = 0; k < n; k++) bad |= (u64)(a.in[0][r * n + k] >= q) | (u64)(a.out[0][r * n + k] >= q);
            if (bad) refuse("add: an operand holds a word that is not a canonical residue of its limb");
        }
    } break;
    case STEP_CLEAR_BITS:
        // e0 = bits (0 .. 63); out[0] [words + 1] in/out, the last word a guard
        need(a.e0 >= 0 && a.e0 <= 63, "clear_bits: bits (e0) outside 0 .. 63");
        need(a.out[0] && a.out_words[0] >= 2, "clear_bits: out[0] [words + 1], words >= 1: wrong size");
        words = a.out_words[0] - 1;
        break;
    case STEP_COPY_JOBS:
        // terms = words per job (even), batch = jobs; in[0] sources [jobs][words] -> out[0] [jobs][words + 2] in/out, two guard words behind each
        need(batch >= 1 && batch <= 64, "copy_jobs: jobs (batch) outside 1 .. 64");
        need(terms >= 2 && terms % 2 == 0, "copy_jobs: words (terms) must be even and at least 2 (the kernel moves 16 bytes at a time)");
        words = terms;
        in_is(0, batch * words, "copy_jobs: in[0] sources [jobs][words]");
        out_is(0, batch * (words + 2), "copy_jobs: out[0] [jobs][words + 2]");
        break;
    case STEP_COPY_SOURCES: {
        // chain_idx = the level (L = chain_idx + 1, words = 2 L n), batch = jobs; in[0] sources [jobs][2][L][n], or null: in place, out[0]
        // is source and destination; in[1] = the report word before, seq (32 bits each) -> out[0] [jobs][2 L n] in/out, out[1] the report word after
        check_level(a.chain_idx);
        L = a.chain_idx + 1;
        need(n % 2 == 0, "copy_sources: an odd ring size");
        need(batch >= 1 && batch <= 64, "copy_sources: jobs (batch) outside 1 .. 64");
        words = 2 * (size_t)L * n;
        if (a.in[0]) in_is(0, batch * words, "copy_sources: in[0] sources [jobs][2][L][n]");
        in_is(1, 2, "copy_sources: in[1] the report word and seq");
        need(!(a.in[1][0] >> 32) && !(a.in[1][1] >> 32), "copy_sources: in[1] holds a word that does not fit 32 bits");
        out_is(0, batch * words, "copy_sources: out[0] [jobs][2][L][n]");
        out_is(1, 1, "copy_sources: out[1] the report word, one word");
    } break;
    case STEP_FILL_RANDOM:
        // in[0] = seed, bound -> out[0] [words + 1] in/out, the last word a guard
        in_is(0, 2, "fill_random: in[0] seed, bound");
        need(a.in[0][1] >= 1, "fill_random: a bound of 0");
        need(a.out[0] && a.out_words[0] >= 2, "fill_random: out[0] [words + 1], words >= 1: wrong size");
        words = a.out_words[0] - 1;
        break;
    case STEP_FILL_BLAKE2XB:
        // in[0] seed [8], in[1] = first, bound -> out[0] [1 + words + 1] in/out, a guard word on both sides
        in_is(0, 8, "fill_blake2xb: in[0] seed [8]");
        in_is(1, 2, "fill_blake2xb: in[1] first, bound");
        need(a.in[1][1] >= 1, "fill_blake2xb: a bound of 0");
        need(a.out[0] && a.out_words[0] >= 3, "fill_blake2xb: out[0] [1 + words + 1], words >= 1: wrong size");
        words = a.out_words[0] - 2;
        need(a.in[1][0] <= ((u64)1 << 62), "fill_blake2xb: first beyond 2^62");
        for (int k = 0; k < 8; k++) seed.w[k] = a.in[0][k];
        break;
    case STEP_SCATTER_SLOTS:
    case STEP_GATHER_SLOTS: {
        // in[0] [batch][n], in[1] a permutation [n] or null: the context's slot map -> out[0] [batch][n] in/out
        need(batch >= 1 && batch <= 64, "scatter_slots / gather_slots: batch outside 1 .. 64");
        in_is(0, batch * n, "scatter_slots / gather_slots: in[0] [batch][n]");
        out_is(0, batch * n, "scatter_slots / gather_slots: out[0] [batch][n]");
        if (!a.in[1]) { need(hp_.batching, "scatter_slots / gather_slots: plain_modulus does not support batching (no slot map of the context's)"); break; }
        in_is(1, n, "scatter_slots / gather_slots: in[1] map [n]");
        std::vector<unsigned char> hit(n, 0);
        map32.resize(n);
        for (size_t i = 0; i < n; i++) {
            need(a.in[1][i] < n, "scatter_slots / gather_slots: a map word at or above n");
            need(!hit[a.in[1][i]], "scatter_slots / gather_slots: the map is not a permutation");
            hit[a.in[1][i]] = 1;
            map32[i] = (u32)a.in[1][i];
        }
    } break;
    case STEP_ALGEBRAIZE:
        // polys = felts, terms = bits per felt, e0 = item_bit_count; in[0] items [count][2] -> out[0] [count * felts + 1] in/out, the last a guard
        need(polys >= 1 && polys <= 64 && terms >= 1 && terms <= 64 && (polys - 1) * terms < 128, "algebraize: felts (polys) or bits per felt (terms) out of range");
        need(e0 >= 1 && e0 <= 128, "algebraize: item_bit_count (e0) outside 1 .. 128");
        need(a.in[0] && a.in_words[0] >= 2 && a.in_words[0] % 2 == 0, "algebraize: in[0] items [count][2], count >= 1: wrong size");
        count = a.in_words[0] / 2;
        out_is(0, count * polys + 1, "algebraize: out[0] [count * felts + 1]");
        break;
    default:                                                           // STEP_PACK_BLOCKS
        // polys = felts, terms = len, e0 = items; in[0] values [batch][n] -> out[0] [batch][items][2] + 1 in/out, the last a guard
        need(batch >= 1 && batch <= 64, "pack_blocks: batch outside 1 .. 64");
        need(polys >= 1 && e0 >= 1 && e0 * polys <= n, "pack_blocks: felts (polys) or items (e0) out of range (items * felts <= n)");
        need(terms >= 2 && terms <= 63, "pack_blocks: len (terms) outside 2 .. 63");
        in_is(0, batch * n, "pack_blocks: in[0] values [batch][n]");
        out_is(0, batch * e0 * 2 + 1, "pack_blocks: out[0] [batch][items][2] + 1");
        break;
    }

    std::vector<CtJob> cj;
    u32 report[2] = { 0, 0 };
    WITH_ARENA({
        cj.clear();                                                    // a retry with a larger arena starts over
        auto up = [&](const u64 *src, size_t w) {
            u64 *d = ws(w + 2);
            if (w) HIP_CHECK(hipMemcpyAsync(d, src, w * sizeof(u64), hipMemcpyHostToDevice, st_));
            return d;
        };
        auto down = [&](u64 *dst, const u64 *src, size_t w) { if (w) HIP_CHECK(hipMemcpyAsync(dst, src, w * sizeof(u64), hipMemcpyDeviceToHost, st_)); };
        auto jobs = [&]() {
            CtJob *d = ws_as<CtJob>(cj.size());
            HIP_CHECK(hipMemcpyAsync(d, cj.data(), cj.size() * sizeof(CtJob), hipMemcpyHostToDevice, st_));
            return static_cast<const CtJob *>(d);
        };
        u64 *o = up(a.out[0], a.out_words[0]);

        switch (a.step) {
        case STEP_ADD:
            launch_add(dlevel(a.chain_idx), o, up(a.in[0], words), (int)polys, n, (int)batch, st_);
            break;
        case STEP_CLEAR_BITS:
            launch_clear_bits(o, words, a.e0, st_);
            break;
        case STEP_COPY_JOBS: {
            const u64 *src = up(a.in[0], a.in_words[0]);
            for (size_t j = 0; j < batch; j++) cj.push_back(CtJob{ src + j * words, o + j * (words + 2) });
            launch_copy_jobs(jobs(), words, (int)batch, st_);
        } break;
        case STEP_COPY_SOURCES: {
            const u64 *src = a.in[0] ? up(a.in[0], a.in_words[0]) : o;
            for (size_t j = 0; j < batch; j++) cj.push_back(CtJob{ src + j * words, o + j * words });
            u32 *bad = ws_as<u32>(2);
            report[0] = (u32)a.in[1][0];
            HIP_CHECK(hipMemcpyAsync(bad, report, sizeof(u32), hipMemcpyHostToDevice, st_));
            launch_copy_sources(jobs(), words, (int)batch, dlevel(a.chain_idx), L, n, bad, (unsigned)a.in[1][1], st_);
            HIP_CHECK(hipMemcpyAsync(report + 1, bad, sizeof(u32), hipMemcpyDeviceToHost, st_));
        } break;
        case STEP_FILL_RANDOM:
            launch_fill_random(o, words, a.in[0][0], a.in[0][1], st_);
            break;
        case STEP_FILL_BLAKE2XB:
            launch_fill_blake2xb(o + 1, words, seed, a.in[1][0], a.in[1][1], st_);
            break;
        case STEP_SCATTER_SLOTS:
        case STEP_GATHER_SLOTS: {
            const u32 *map = reinterpret_cast<const uint32_t *>(d_slot_map_.p());
            if (a.in[1]) {
                u32 *m = ws_as<u32>(n);
                HIP_CHECK(hipMemcpyAsync(m, map32.data(), n * sizeof(u32), hipMemcpyHostToDevice, st_));
                map = m;
            }
            const u64 *in = up(a.in[0], a.in_words[0]);
            if (a.step == STEP_SCATTER_SLOTS) launch_scatter_slots(in, map, o, n, (int)batch, st_);
            else launch_gather_slots(in, map, o, n, (int)batch, st_);
        } break;
        case STEP_ALGEBRAIZE:
            launch_algebraize(reinterpret_cast<const unsigned char *>(up(a.in[0], a.in_words[0])), count, (u32)polys, (u32)terms, (u32)e0, o, st_);
            break;
        default:                                                       // STEP_PACK_BLOCKS
            launch_pack_blocks(up(a.in[0], a.in_words[0]), n, (u32)e0, (u32)polys, (u32)terms, o, (int)batch, st_);
            break;
        }
        down(a.out[0], o, a.out_words[0]);
        sync();
        if (a.step == STEP_COPY_SOURCES) a.out[1][0] = report[1];
    });
}

} // namespace apsu_he
