// Stand-alone driver of the plaintext evaluation's lane functions and of the self-test reports' reduction (apsu_amd/csrc/bin_eval.h:
// eval_walk and its bounds as k_bins_eval and emu_bins_eval call them, self_test_reduce), meant to be built with
// -fsanitize=address,undefined (tests/test_bundle_eval_cpu.py).  Every array handed over is an exact-size heap allocation, so a read or
// write past its end is seen; the expected values are Horner walks in 128-bit arithmetic.  Prints "ok" and returns 0, or says what differed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "bin_eval.h"

using namespace apsu_he;

namespace {

[[noreturn]] void fail(const std::string &what)
{
    std::fprintf(stderr, "FAILED: %s\n", what.c_str());
    std::exit(1);
}
#define EXPECT(cond) do { if (!(cond)) fail(std::string(#cond) + " (line " + std::to_string(__LINE__) + ")"); } while (0)

uint64_t next(uint64_t &s) { s += 0x9e3779b97f4a7c15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }

template <class T> std::unique_ptr<T[]> exact(size_t count) { return std::unique_ptr<T[]>(new T[count ? count : 1]); }

// floor(2^128 / q) as the two words of Mod (q < 2^63)
Mod mod_of(uint64_t q)
{
    const unsigned __int128 one = (unsigned __int128)1 << 64;
    const uint64_t r1 = (uint64_t)(one / q), rem = (uint64_t)(one % q);
    return Mod{ q, (uint64_t)(((unsigned __int128)rem << 64) / q), r1 };
}

// the kernel's structure: per tile the largest count over its lanes, then every lane's walk from there
int emu_bins_eval(uint64_t t_, const uint64_t *poly, size_t n, uint32_t rows, const uint64_t *x, const uint64_t *mask, int wide, uint64_t *out,
                  unsigned char *is_bin, uint32_t *walked)
{
    for (size_t s = 0; s < n; s++)
        if (x[s] >= t_ || (mask && mask[s] >= t_)) return -1;
    const Mod t = mod_of(t_);
    const bool narrow = !wide && merge_narrow(merge_bits(t_));
    auto counts = exact<uint32_t>(n);
    for (size_t s = 0; s < n; s++) {
        int top = (int)rows - 1;
        while (top >= 0 && poly[(size_t)top * n + s] == 0) top--;
        counts[s] = bin_count_of(top);
    }
    for (size_t tile = 0; tile * EVAL_LANES < n; tile++) {
        int top = -1;
        for (int lane = 0; lane < EVAL_LANES; lane++) {
            const size_t slot = tile * EVAL_LANES + lane;
            const int c = eval_count_top(slot < n ? counts[slot] : LOOKUP_NONE);
            top = c > top ? c : top;
        }
        const int d0 = eval_walk_top(top, rows);
        if (walked) walked[tile] = (uint32_t)(d0 + 1);
        for (int lane = 0; lane < EVAL_LANES; lane++) {
            const size_t slot = tile * EVAL_LANES + lane;
            if (slot >= n) continue;
            const uint64_t acc = narrow ? eval_walk<true>(poly + slot, n, d0, x[slot], t) : eval_walk<false>(poly + slot, n, d0, x[slot], t);
            out[slot] = eval_finish(acc, mask ? mask[slot] : 0, t);
            if (is_bin) is_bin[slot] = eval_is_bin(counts[slot]) ? 1 : 0;
        }
    }
    return 0;
}

int emu_self_test_report_bytes() { return (int)sizeof(SelfTestReport); }
void emu_self_test_reduce(const SelfTestReport *parts, int count, SelfTestReport *out)
{
    SelfTestReport r = self_test_empty();
    for (int i = 0; i < count; i++) self_test_reduce(r, parts[i]);
    *out = r;
}

void one_shape(uint64_t t, size_t n, uint32_t rows, bool masked, uint64_t &seed)
{
    auto poly = exact<uint64_t>((size_t)rows * n);
    auto x = exact<uint64_t>(n), mask = exact<uint64_t>(n), out = exact<uint64_t>(n);
    auto is_bin = exact<unsigned char>(n);
    const size_t tiles = (n + EVAL_LANES - 1) / EVAL_LANES;
    auto walked = exact<uint32_t>(tiles);
    // tile 0: every coefficient t - 1 (the largest sums); tile 1: short bins (count <= 1) and a slot with the zero polynomial; the rest random
    for (uint32_t d = 0; d < rows; d++)
        for (size_t s = 0; s < n; s++) {
            uint64_t v = next(seed) % t;
            if (s < 64) v = t - 1;
            else if (s < 128) v = d == 0 ? (s == 70 ? 0 : v) : d == 1 && s % 2 ? 1 : 0;
            poly[(size_t)d * n + s] = v;
        }
    const uint64_t pts[4] = { 0, 1, t - 1, t / 2 };
    for (size_t s = 0; s < n; s++) { x[s] = s % 5 == 4 ? next(seed) % t : pts[s % 5]; mask[s] = s % 3 ? next(seed) % t : t - 1; out[s] = ~(uint64_t)0; is_bin[s] = 0xEE; }
    for (int wide = 0; wide < 2; wide++) {
        EXPECT(emu_bins_eval(t, poly.get(), n, rows, x.get(), masked ? mask.get() : nullptr, wide, out.get(), is_bin.get(), walked.get()) == 0);
        for (size_t s = 0; s < n; s++) {
            unsigned __int128 acc = 0;
            bool any = false;
            for (int d = (int)rows - 1; d >= 0; d--) { acc = (acc * x[s] + poly[(size_t)d * n + s]) % t; any |= poly[(size_t)d * n + s] != 0; }
            if (masked) acc = (acc + mask[s]) % t;
            EXPECT(out[s] == (uint64_t)acc);
            EXPECT(is_bin[s] == (any ? 1 : 0));
        }
        EXPECT(walked[0] == rows);
        if (tiles > 1 && n >= 128) EXPECT(walked[1] == (rows > 1 ? 2u : 1u));
    }
    x[n - 1] = t;                                                      // not reduced: refused, nothing else read
    EXPECT(emu_bins_eval(t, poly.get(), n, rows, x.get(), nullptr, 0, out.get(), nullptr, nullptr) == -1);
}

void reports()
{
    EXPECT(emu_self_test_report_bytes() == (int)sizeof(SelfTestReport));
    SelfTestReport none;
    emu_self_test_reduce(nullptr, 0, &none);
    EXPECT(none.bundles == 0 && none.first_bundle == -1 && none.min_budget_bundle == -1 && none.mismatches == 0);
    auto parts = exact<SelfTestReport>(3);
    parts[0] = self_test_empty();
    parts[1] = self_test_empty();
    parts[2] = self_test_empty();
    parts[0].bundles = 2; parts[0].slots = 128; parts[0].min_budget_bits = 7; parts[0].min_budget_bundle = 4; parts[0].he_ms = 2; parts[0].plain_ms = 1;
    parts[1].bundles = 1; parts[1].slots = 64; parts[1].mismatches = 3; parts[1].first_bundle = 5; parts[1].first_slot = 9; parts[1].first_got = 1;
    parts[1].first_expected = 2; parts[1].min_budget_bits = 0; parts[1].min_budget_bundle = 5; parts[1].he_ms = 1; parts[1].plain_ms = 3;
    SelfTestReport all;
    emu_self_test_reduce(parts.get(), 3, &all);
    EXPECT(all.bundles == 3 && all.slots == 192 && all.mismatches == 3);
    EXPECT(all.first_bundle == 5 && all.first_slot == 9 && all.first_got == 1 && all.first_expected == 2);
    EXPECT(all.min_budget_bits == 0 && all.min_budget_bundle == 5 && all.he_ms == 2 && all.plain_ms == 3);
}

}  // namespace

int main()
{
    uint64_t seed = 1;
    const uint64_t moduli[] = { 40961, 65537, 1032193, 4294967291ull, 4294967311ull, ((uint64_t)1 << 60) - 93 };
    for (uint64_t t : moduli)
        for (size_t n : { (size_t)64, (size_t)130 })
            for (uint32_t rows : { 1u, 2u, (uint32_t)EVAL_ROWS - 1, (uint32_t)EVAL_ROWS, (uint32_t)EVAL_ROWS + 1, (uint32_t)EVAL_ROWS + 2, 3u * EVAL_ROWS + 1 })
                for (int masked = 0; masked < 2; masked++) one_shape(t, n, rows, masked != 0, seed);
    reports();
    std::puts("ok");
    return 0;
}
