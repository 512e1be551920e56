// One resident-database kernel at a time on caller-chosen words (Engine::debug_run_step from STEP_POLYN_WITH_ROOTS on; include/apsu_he.h).
// As engine_steps.cpp does for the element-wise HE kernels: a step copies host arrays up in the layout device.h documents for its
// launcher, calls THE launch_* function the engine calls with make_mod(t) and the context's n -- so the launcher's choice of template
// instance is part of what runs -- synchronises and copies back.  32-bit and byte arrays (counts, touched, occ, idx, tops, flags)
// travel as 64-bit words and are narrowed here.  Whatever a launcher's input contract (device.h) does not admit is refused before
// anything is launched.  For the tests; nothing on the query path calls it.
#include "engine_impl.h"

#include <functional>
#include <list>
#include <string>

namespace apsu_he {

namespace {

[[noreturn]] void refuse(const std::string &why) { throw std::invalid_argument("debug_run_step: " + why); }
void need(bool ok, const char *why) { if (!ok) refuse(why); }

// the index of the highest non-zero word of column s of poly[rows][n], -1 for none
int column_top(const u64 *poly, size_t n, size_t rows, size_t s)
{
    int top = (int)rows - 1;
    while (top >= 0 && poly[(size_t)top * n + s] == 0) top--;
    return top;
}

void canonical_column(const u64 *poly, size_t n, size_t rows, size_t s, u64 t, const char *what)
{
    u64 bad = 0;
    for (size_t d = 0; d < rows; d++) bad |= (u64)(poly[d * n + s] >= t);
    if (bad) refuse(std::string(what) + " holds a word that is not a canonical residue of plain_modulus");
}

void canonical_words(const u64 *x, size_t words, u64 t, const char *what)
{
    u64 bad = 0;
    for (size_t i = 0; i < words; i++) bad |= (u64)(x[i] >= t);
    if (bad) refuse(std::string(what) + " holds a word that is not a canonical residue of plain_modulus");
}

} // namespace

void Engine::debug_run_db_step(const StepArgs &a)
{
    const size_t n = hp_.n, tiles = (n + 63) / 64;
    const u64 t = hp_.t;
    const Mod T = make_mod(t);
    const size_t terms = a.terms > 0 ? (size_t)a.terms : 0, polys = a.polys > 0 ? (size_t)a.polys : 0, batch = a.batch > 0 ? (size_t)a.batch : 0;
    const size_t e0 = a.e0 > 0 ? (size_t)a.e0 : 0;
    constexpr size_t ROWS_MAX = (size_t)1 << 20;                       // far above every shape a BinBundle has; keeps rows * n small
    auto in_is = [&](int i, size_t words, const char *what) { if (!a.in[i] || a.in_words[i] != words) refuse(std::string(what) + ": wrong size"); };
    auto out_is = [&](int i, size_t words, const char *what) { if (!a.out[i] || a.out_words[i] != words) refuse(std::string(what) + ": wrong size"); };
    auto fits32 = [&](const u64 *x, size_t words, const char *what) {
        u64 bad = 0;
        for (size_t i = 0; i < words; i++) bad |= x[i] >> 32;
        if (bad) refuse(std::string(what) + " holds a word that does not fit 32 bits");
    };
    auto fits8 = [&](const u64 *x, size_t words, const char *what) {
        u64 bad = 0;
        for (size_t i = 0; i < words; i++) bad |= x[i] >> 8;
        if (bad) refuse(std::string(what) + " holds a word that does not fit a byte");
    };

    // host copies of the narrowed arrays and the widening of what comes back: both outlive the queued copies (the call ends with a sync)
    std::list<std::vector<u32>> keep32;
    std::list<std::vector<unsigned char>> keep8;
    std::vector<std::function<void()>> after;

    WITH_ARENA({
        keep32.clear(); keep8.clear(); after.clear();                  // a retry with a larger arena starts over
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
            if (words) HIP_CHECK(hipMemcpyAsync(d, h.data(), words * sizeof(u32), hipMemcpyHostToDevice, st_));
            return d;
        };
        auto up8 = [&](const u64 *src, size_t words) {
            keep8.emplace_back(words);
            std::vector<unsigned char> &h = keep8.back();
            for (size_t i = 0; i < words; i++) h[i] = (unsigned char)src[i];
            unsigned char *d = ws_as<unsigned char>(words, 1);
            if (words) HIP_CHECK(hipMemcpyAsync(d, h.data(), words, hipMemcpyHostToDevice, st_));
            return d;
        };
        auto down = [&](u64 *dst, const u64 *src, size_t words) { if (words) HIP_CHECK(hipMemcpyAsync(dst, src, words * sizeof(u64), hipMemcpyDeviceToHost, st_)); };
        auto down32 = [&](u64 *dst, const u32 *src, size_t words) {
            keep32.emplace_back(words);
            std::vector<u32> *h = &keep32.back();
            if (words) HIP_CHECK(hipMemcpyAsync(h->data(), src, words * sizeof(u32), hipMemcpyDeviceToHost, st_));
            after.push_back([=] { for (size_t i = 0; i < words; i++) dst[i] = (*h)[i]; });
        };
        auto down8 = [&](u64 *dst, const unsigned char *src, size_t words) {
            keep8.emplace_back(words);
            std::vector<unsigned char> *h = &keep8.back();
            if (words) HIP_CHECK(hipMemcpyAsync(h->data(), src, words, hipMemcpyDeviceToHost, st_));
            after.push_back([=] { for (size_t i = 0; i < words; i++) dst[i] = (*h)[i]; });
        };

        switch (a.step) {
        case STEP_POLYN_WITH_ROOTS: {
            // polys = bins, terms = stride, e0 = max_deg; in[0] roots [bins][stride], in[1] counts [bins] -> out[0] poly [max_deg + 1][n]
            const size_t bins = polys, stride = terms, max_deg = e0;
            need(bins >= 1 && bins <= n, "polyn_with_roots: bins (polys) out of range (1 .. n)");
            need(stride >= 1 && stride < ROWS_MAX && max_deg < ROWS_MAX, "polyn_with_roots: stride (terms) or max_deg (e0) out of range");
            in_is(0, bins * stride, "polyn_with_roots: in[0] roots [bins][stride]");
            in_is(1, bins, "polyn_with_roots: in[1] counts [bins]");
            out_is(0, (max_deg + 1) * n, "polyn_with_roots: out[0] poly [max_deg + 1][n]");
            for (size_t s = 0; s < bins; s++) {
                const u64 c = a.in[1][s];
                need(c <= stride && c <= max_deg, "polyn_with_roots: a count exceeds stride or max_deg");
                canonical_words(a.in[0] + s * stride, (size_t)c, t, "polyn_with_roots: in[0] (a bin's roots below its count)");
            }
            const u64 *dr = up(a.in[0], a.in_words[0]);
            const u32 *dc = up32(a.in[1], bins);
            u64 *o = ws(a.out_words[0]);
            launch_polyn_with_roots(dr, dc, (u32)bins, (u32)stride, (u32)max_deg, T, o, n, st_);
            down(a.out[0], o, a.out_words[0]);
        } break;
        case STEP_BINS_UPDATE: {
            // terms = rows, batch = bins, polys = ins_stride, e0 = rem_stride; in[0] touched [n_touched], in[1] ins [bins][ins_stride],
            // in[2] ins_counts [bins] (both or neither), in[3] rem [bins][rem_stride], in[4] rem_counts [bins] (both or neither);
            // out[0] poly [rows][n], updated in place; out[1] counts_out [n_touched] (in: what a failing wave leaves), status[0], status[1]
            const size_t rows = terms, bins = batch, is = polys, rs = e0, nt = a.in_words[0];
            need(rows >= 1 && rows < ROWS_MAX, "bins_update: rows (terms) out of range");
            need(bins >= 1 && bins <= n, "bins_update: bins (batch) out of range (1 .. n)");
            need(a.in[0] && nt >= 1 && nt <= bins, "bins_update: in[0] touched: 1 .. bins entries");
            need((a.in[1] == nullptr) == (a.in[2] == nullptr) && (a.in[3] == nullptr) == (a.in[4] == nullptr), "bins_update: a root list and its counts are given together or not at all");
            if (a.in[1]) { need(is >= 1 && is < ROWS_MAX, "bins_update: ins_stride (polys) out of range"); in_is(1, bins * is, "bins_update: in[1] ins [bins][ins_stride]"); in_is(2, bins, "bins_update: in[2] ins_counts [bins]"); }
            if (a.in[3]) { need(rs >= 1 && rs < ROWS_MAX, "bins_update: rem_stride (e0) out of range"); in_is(3, bins * rs, "bins_update: in[3] rem [bins][rem_stride]"); in_is(4, bins, "bins_update: in[4] rem_counts [bins]"); }
            out_is(0, rows * n, "bins_update: out[0] poly [rows][n]");
            out_is(1, nt + 2, "bins_update: out[1] counts_out [n_touched], status [2]");
            fits32(a.out[1], nt, "bins_update: out[1] (counts_out beforehand)");
            std::vector<bool> seen(bins, false);
            for (size_t w = 0; w < nt; w++) {
                const u64 s = a.in[0][w];
                need(s < bins, "bins_update: a touched bin is not below bins");
                need(!seen[s], "bins_update: a bin is named twice in touched (two waves would update one column)");
                seen[s] = true;
                const u64 ni = a.in[2] ? a.in[2][s] : 0, nr = a.in[4] ? a.in[4][s] : 0;
                need(ni <= is && nr <= rs, "bins_update: a bin's count exceeds its stride");
                if (ni) canonical_words(a.in[1] + s * is, (size_t)ni, t, "bins_update: in[1] (a bin's insertions)");
                if (nr) canonical_words(a.in[3] + s * rs, (size_t)nr, t, "bins_update: in[3] (a bin's removals)");
                canonical_column(a.out[0], n, rows, s, t, "bins_update: out[0] (a touched column)");
                const int top = column_top(a.out[0], n, rows, s);
                need(top < 0 || (size_t)top + ni <= rows - 1 + std::min<u64>(nr, (u64)top), "bins_update: a count >= rows after the insertions (the bin would outgrow the array)");
            }
            const u32 *dt = up32(a.in[0], nt);
            const u64 *di = a.in[1] ? up(a.in[1], a.in_words[1]) : ws(1), *dr = a.in[3] ? up(a.in[3], a.in_words[3]) : ws(1);
            const u32 *dic = a.in[2] ? up32(a.in[2], bins) : nullptr, *drc = a.in[4] ? up32(a.in[4], bins) : nullptr;
            u64 *poly = up(a.out[0], a.out_words[0]);
            u32 *dnew = up32(a.out[1], nt);
            u64 *status = ws(2);
            HIP_CHECK(hipMemsetAsync(status, 0xff, 2 * sizeof(u64), st_));
            launch_bins_update(dt, (u32)nt, di, dic, (u32)is, dr, drc, (u32)rs, T, poly, n, (u32)rows, dnew, status, st_);
            down(a.out[0], poly, a.out_words[0]);
            down32(a.out[1], dnew, nt);
            down(a.out[1] + nt, status, 2);
        } break;
        case STEP_BIN_COUNTS:
        case STEP_POLY_DEGREE: {
            // terms = rows; in[0] poly [rows][n] (any words: only tested for zero) -> out[0] counts [n] / the degree (one word)
            const size_t rows = terms;
            need(rows >= 1 && rows < ROWS_MAX, "bin_counts / poly_degree: rows (terms) out of range");
            in_is(0, rows * n, "bin_counts / poly_degree: in[0] poly [rows][n]");
            const u64 *poly = nullptr;
            if (a.step == STEP_BIN_COUNTS) {
                out_is(0, n, "bin_counts: out[0] counts [n]");
                poly = up(a.in[0], a.in_words[0]);
                u32 *dc = ws_as<u32>(n, 1);
                launch_bin_counts(poly, n, (u32)rows, dc, st_);
                down32(a.out[0], dc, n);
            } else {
                out_is(0, 1, "poly_degree: out[0] one word");
                poly = up(a.in[0], a.in_words[0]);
                u64 *o = ws(1);
                HIP_CHECK(hipMemsetAsync(o, 0, sizeof(u64), st_));
                launch_poly_degree(poly, n, (u32)rows, o, st_);
                down(a.out[0], o, 1);
            }
        } break;
        case STEP_UNLIFT: {
            // in[0] residues of q_0 as the lift stores them -> out[0] values mod t, the same size
            const u64 q0 = hp_.key_q[0];
            need(a.in[0] && a.in_words[0] >= 1, "unlift: in[0] is empty");
            out_is(0, a.in_words[0], "unlift: out[0] as many words as in[0]");
            need(q0 > 2 * t, "unlift: q_0 <= 2 * plain_modulus");
            u64 bad = 0;
            for (size_t i = 0; i < a.in_words[0]; i++) { const u64 x = a.in[0][i]; bad |= (u64)(x >= q0 || (x >= t && x < q0 - t)); }
            need(!bad, "unlift: in[0] holds a word that is neither a value below plain_modulus nor a lifted one (q_0 - t .. q_0 - 1)");
            u64 *x = up(a.in[0], a.in_words[0]);
            launch_unlift(x, a.in_words[0], t, q0, st_);
            down(a.out[0], x, a.in_words[0]);
        } break;
        case STEP_BINS_LOOKUP: {
            // terms = degree; in[0] poly [degree + 1][n]; out[0] flags [parts], one word each (in: what an unnamed part keeps).
            // Without STEP_PLAN: polys = F, in[1] felts [count][F], in[2] start [count] -> lookup_plan with LOOKUP_R rows per work item.
            // With STEP_PLAN the caller's plan: in[1] work [n_work][4] (tile, row0, nrows, 0), in[2] pts [rows][64], in[3] idx [rows][64].
            const size_t degree = terms, parts = a.out_words[0];
            need(degree < ROWS_MAX, "bins_lookup: degree (terms) out of range");
            in_is(0, (degree + 1) * n, "bins_lookup: in[0] poly [degree + 1][n]");
            need(a.out[0] && parts >= 1 && parts < LOOKUP_NONE, "bins_lookup: out[0] flags: at least one part");
            canonical_words(a.in[0], a.in_words[0], t, "bins_lookup: in[0]");
            fits8(a.out[0], parts, "bins_lookup: out[0] (flags beforehand)");
            LookupPlan plan;
            if (!(a.flags & STEP_PLAN)) {
                const size_t F = polys;
                need(F >= 1 && F <= n && a.in[1] && a.in_words[1] == parts && parts % F == 0, "bins_lookup: in[1] felts [count][F] with count * F = the parts of out[0]");
                const size_t count = parts / F;
                in_is(2, count, "bins_lookup: in[2] start [count]");
                canonical_words(a.in[1], parts, t, "bins_lookup: in[1]");
                std::vector<u32> start(count);
                for (size_t e = 0; e < count; e++) { need(a.in[2][e] + F <= n, "bins_lookup: start bin + F exceeds n"); start[e] = (u32)a.in[2][e]; }
                plan = lookup_plan(a.in[1], start.data(), count, (u32)F, n, LOOKUP_R);
            } else {
                need(a.in[1] && a.in_words[1] >= 4 && a.in_words[1] % 4 == 0, "bins_lookup: in[1] work [n_work][4]");
                need(a.in[2] && a.in_words[2] >= 64 && a.in_words[2] % 64 == 0, "bins_lookup: in[2] pts [rows][64]");
                in_is(3, a.in_words[2], "bins_lookup: in[3] idx [rows][64]");
                const size_t rows = a.in_words[2] / 64;
                canonical_words(a.in[2], a.in_words[2], t, "bins_lookup: in[2]");
                std::vector<bool> seen(parts, false);
                plan.pts.assign(a.in[2], a.in[2] + a.in_words[2]);
                plan.idx.resize(a.in_words[3]);
                for (size_t i = 0; i < a.in_words[3]; i++) {
                    const u64 p = a.in[3][i];
                    need(p == LOOKUP_NONE || p < parts, "bins_lookup: an index entry is neither LOOKUP_NONE nor a part");
                    if (p != LOOKUP_NONE) { need(!seen[p], "bins_lookup: a part is named twice"); seen[p] = true; }
                    plan.idx[i] = (u32)p;
                }
                for (size_t w = 0; w < a.in_words[1] / 4; w++) {
                    const u64 *k = a.in[1] + 4 * w;
                    need(k[0] < tiles && k[2] >= 1 && k[2] <= (u64)LOOKUP_R && k[1] < rows && k[1] + k[2] <= rows, "bins_lookup: a work item outside the tiles, the rows or 1 .. LOOKUP_R");
                    plan.work.push_back(LookupWork{ (u32)k[0], (u32)k[1], (u32)k[2], 0 });
                }
            }
            const u64 *poly = up(a.in[0], a.in_words[0]);
            LookupWork *dwork = ws_as<LookupWork>(plan.work.size(), 1);
            u64 *dpts = ws(plan.pts.size() + 1);
            u32 *didx = ws_as<u32>(plan.idx.size(), 1);
            keep32.emplace_back(plan.idx);
            const std::vector<u32> &hidx = keep32.back();
            keep32.emplace_back(plan.work.size() * 4);
            std::vector<u32> &hwork = keep32.back();
            for (size_t w = 0; w < plan.work.size(); w++) { hwork[4 * w] = plan.work[w].tile; hwork[4 * w + 1] = plan.work[w].row0; hwork[4 * w + 2] = plan.work[w].nrows; hwork[4 * w + 3] = 0; }
            static_assert(sizeof(LookupWork) == 16, "LookupWork is four 32-bit words");
            if (!plan.work.empty()) {
                HIP_CHECK(hipMemcpyAsync(dwork, hwork.data(), hwork.size() * sizeof(u32), hipMemcpyHostToDevice, st_));
                HIP_CHECK(hipMemcpyAsync(didx, hidx.data(), hidx.size() * sizeof(u32), hipMemcpyHostToDevice, st_));
                HIP_CHECK(hipMemcpyAsync(dpts, plan.pts.data(), plan.pts.size() * sizeof(u64), hipMemcpyHostToDevice, st_));
            }
            unsigned char *dflags = up8(a.out[0], parts);
            launch_bins_lookup(dwork, (u32)plan.work.size(), dpts, didx, T, poly, n, (u32)degree, dflags, st_);
            sync();                                                    // (plan.pts is this block's own)
            down8(a.out[0], dflags, parts);
        } break;
        case STEP_BINS_MERGE: {
            // terms = rows of C; in[0] A [rowsA][n], in[1] topsA [tiles], in[2] B [rowsB][n], in[3] topsB [tiles] (tops: two's complement,
            // -1 = no bin in the tile) -> out[0] C [rows][n]
            const size_t rows = terms;
            need(rows >= 1 && rows < ROWS_MAX, "bins_merge: rows (terms) out of range");
            need(a.in[0] && a.in_words[0] >= n && a.in_words[0] % n == 0 && a.in[2] && a.in_words[2] >= n && a.in_words[2] % n == 0, "bins_merge: in[0] A [rowsA][n], in[2] B [rowsB][n]");
            in_is(1, tiles, "bins_merge: in[1] topsA [tiles]");
            in_is(3, tiles, "bins_merge: in[3] topsB [tiles]");
            out_is(0, rows * n, "bins_merge: out[0] C [rows][n]");
            keep32.emplace_back(2 * tiles);
            std::vector<u32> &htops = keep32.back();
            for (int side = 0; side < 2; side++) {
                const u64 *X = a.in[2 * side], *tp = a.in[2 * side + 1];
                const int64_t have = (int64_t)(a.in_words[2 * side] / n);
                for (size_t tl = 0; tl < tiles; tl++) {
                    const int64_t top = (int64_t)tp[tl];
                    need(top >= -1 && top < have && top < (int64_t)ROWS_MAX, "bins_merge: a tile's top is outside -1 .. rows of its array - 1");
                    htops[side * tiles + tl] = (u32)(int)top;
                    const size_t lanes = std::min<size_t>(64, n - tl * 64);
                    for (int64_t d = 0; d <= top; d++) canonical_words(X + (size_t)d * n + tl * 64, lanes, t, "bins_merge: an operand (rows up to its tile's top)");
                }
            }
            const u64 *dA = up(a.in[0], a.in_words[0]), *dB = up(a.in[2], a.in_words[2]);
            int *dtops = ws_as<int>(2 * tiles, 1);
            HIP_CHECK(hipMemcpyAsync(dtops, htops.data(), 2 * tiles * sizeof(u32), hipMemcpyHostToDevice, st_));
            u64 *o = ws(a.out_words[0]);
            launch_bins_merge(dA, dtops, dB, dtops + tiles, T, o, n, (u32)rows, st_);
            down(a.out[0], o, a.out_words[0]);
        } break;
        case STEP_BINS_ROWS: {
            // terms = rows, polys = bins; in[0] poly [rows][n] (any words), in[1] counts [n] (LOOKUP_NONE: not a bin) -> out[0] the ragged rows
            // (at least off[bins] words; in: what the words nobody writes keep), out[1] off [bins + 1]
            const size_t rows = terms, bins = polys;
            need(rows >= 1 && rows < ROWS_MAX, "bins_rows: rows (terms) out of range");
            need(bins >= 1 && bins <= n, "bins_rows: bins (polys) out of range (1 .. n)");
            in_is(0, rows * n, "bins_rows: in[0] poly [rows][n]");
            in_is(1, n, "bins_rows: in[1] counts [n]");
            out_is(1, bins + 1, "bins_rows: out[1] off [bins + 1]");
            fits32(a.in[1], n, "bins_rows: in[1]");
            std::vector<u32> counts(n);
            for (size_t s = 0; s < n; s++) counts[s] = (u32)a.in[1][s];
            std::vector<u64> off;
            try { off = rows_offsets(counts.data(), (u32)bins, (u32)rows); } catch (const std::invalid_argument &e) { refuse(std::string("bins_rows: ") + e.what()); }
            const std::vector<int> tops = rows_tile_tops(counts.data(), n, (u32)bins);
            need(a.out[0] && a.out_words[0] >= off[bins], "bins_rows: out[0] holds fewer than off[bins] words");
            const u64 *poly = up(a.in[0], a.in_words[0]);
            const u32 *dc = up32(a.in[1], n);
            const u64 *doff = up(off.data(), off.size());
            int *dtops = ws_as<int>(tops.size(), 1);
            HIP_CHECK(hipMemcpyAsync(dtops, tops.data(), tops.size() * sizeof(int), hipMemcpyHostToDevice, st_));
            u64 *o = up(a.out[0], a.out_words[0]);
            launch_bins_rows(poly, n, (u32)rows, dc, doff, dtops, (u32)bins, o, st_);
            sync();                                                    // (off and tops are this block's own)
            down(a.out[0], o, a.out_words[0]);
            for (size_t s = 0; s <= bins; s++) a.out[1][s] = off[s];
        } break;
        case STEP_BINS_EVAL: {
            // terms = rows; in[0] poly [rows][n], in[1] counts [n], in[2] x [n], in[3] mask [n] or null (x, mask: any word, one >= t raises
            // bad) -> out[0] [n] (in: poison), out[1] is_bin [n] (in: poison), bad (one word)
            const size_t rows = terms;
            need(rows >= 1 && rows < ROWS_MAX, "bins_eval: rows (terms) out of range");
            in_is(0, rows * n, "bins_eval: in[0] poly [rows][n]");
            in_is(1, n, "bins_eval: in[1] counts [n]");
            in_is(2, n, "bins_eval: in[2] x [n]");
            if (a.in[3]) in_is(3, n, "bins_eval: in[3] mask [n]");
            out_is(0, n, "bins_eval: out[0] [n]");
            out_is(1, n + 1, "bins_eval: out[1] is_bin [n], bad");
            canonical_words(a.in[0], a.in_words[0], t, "bins_eval: in[0]");
            fits32(a.in[1], n, "bins_eval: in[1]");
            fits8(a.out[1], n, "bins_eval: out[1] (is_bin beforehand)");
            const u64 *poly = up(a.in[0], a.in_words[0]), *x = up(a.in[2], n), *mask = a.in[3] ? up(a.in[3], n) : nullptr;
            const u32 *dc = up32(a.in[1], n);
            u64 *o = up(a.out[0], n);
            unsigned char *dbin = up8(a.out[1], n);
            u32 *bad = ws_as<u32>(1, 1);
            HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(u64), st_));
            launch_bins_eval(poly, n, (u32)rows, dc, x, mask, T, o, dbin, bad, st_);
            down(a.out[0], o, n);
            down8(a.out[1], dbin, n);
            down32(a.out[1] + n, bad, 1);
        } break;
        case STEP_EVAL_COMPARE: {
            // polys = count; in[0] got [count][n], in[1] want [count][n] -> out[0] mismatches, the lowest (position << 32 | slot) or ~0
            const size_t count = polys;
            need(count >= 1 && count <= 65535, "eval_compare: count (polys) out of range (1 .. 65535)");
            in_is(0, count * n, "eval_compare: in[0] got [count][n]");
            in_is(1, count * n, "eval_compare: in[1] want [count][n]");
            out_is(0, 2, "eval_compare: out[0] status [2]");
            const u64 *g = up(a.in[0], a.in_words[0]), *w = up(a.in[1], a.in_words[1]);
            const u64 init[2] = { 0, EVAL_NO_MISMATCH };
            u64 *status = up(init, 2);
            sync();                                                    // (init is this block's own)
            launch_eval_compare(g, w, n, (u32)count, status, st_);
            down(a.out[0], status, 2);
        } break;
        case STEP_ROOTS: {
            // terms = rows, e0 = hstride, batch = workgroups of the persistent kernel (0: the engine's own number); STEP_COMPOSED: gather +
            // transform + scan per coset instead.  in[0] poly [rows][n]; the occupied bins are the columns whose top non-zero row is >= 1, in
            // slot order.  out[0] hits [n_occ][hstride] (in: poison), out[1] found [n_occ], mult [n_occ][hstride] (in: poison)
            const size_t rows = terms, hstride = e0;
            need(hp_.batching, "roots: plain_modulus does not support batching");
            need((t - 1) % (2 * n) == 0 && (t - 1) / n <= ROOTS_MAX_COSETS, "roots: plain_modulus has more than ROOTS_MAX_COSETS cosets of the transform's points");
            need(rows >= 1 && rows <= n, "roots: a degree >= n does not fit one transform (rows = terms in 1 .. n)");
            in_is(0, rows * n, "roots: in[0] poly [rows][n]");
            canonical_words(a.in[0], a.in_words[0], t, "roots: in[0]");
            const bool has_kernel = bin_roots_has_kernel(hp_.logn), kernel = has_kernel && !(a.flags & STEP_COMPOSED);
            std::vector<u64> counts(n);
            std::vector<u64> occ;
            size_t most = 0;
            for (size_t s = 0; s < n; s++) {
                const int top = column_top(a.in[0], n, rows, s);
                counts[s] = bin_count_of(top);
                if (top >= 1) { occ.push_back(s); most = std::max(most, (size_t)top); }
            }
            const size_t n_occ = occ.size();
            need(n_occ >= 1, "roots: no occupied bin");
            need(hstride >= most && hstride <= n, "roots: hstride (e0) is below the largest count, or above n");
            out_is(0, n_occ * hstride, "roots: out[0] hits [n_occ][hstride]");
            out_is(1, n_occ + n_occ * hstride, "roots: out[1] found [n_occ], mult [n_occ][hstride]");
            fits32(a.out[1] + n_occ, n_occ * hstride, "roots: out[1] (mult beforehand)");
            roots_tables();
            const u32 cosets = roots_coset_count(t, n);
            const u32 *step = reinterpret_cast<const u32 *>(d_roots_step_.p());
            const u64 *pts = d_roots_pts_.u();
            u64 *poly = up(a.in[0], a.in_words[0]);
            const u32 *dcounts = up32(counts.data(), n), *docc = up32(occ.data(), n_occ);
            u32 *dfound = ws_as<u32>(n_occ, 1), *dmult = up32(a.out[1] + n_occ, n_occ * hstride);
            u64 *dhits = up(a.out[0], a.out_words[0]);
            HIP_CHECK(hipMemsetAsync(dfound, 0, n_occ * sizeof(u32), st_));
            sync();                                                    // (counts and occ are this block's own)
            if (kernel) {
                const u32 slots = bin_roots_wg_slots(hp_.logn);
                const RootsGrid grid = roots_grid((u32)n_occ, cosets, slots);
                need(batch <= slots, "roots: more workgroups (batch) than the device holds at once");
                const u32 wgs = (u32)std::min<u64>((u64)n_occ * grid.blocks, batch ? batch : slots);
                u64 *wrows = ws((size_t)wgs * n);
                u32 *vrows = ws_as<u32>((size_t)wgs * n);
                launch_bin_roots(hp_.logn, poly, docc, dcounts, (u32)n_occ, grid, cosets, wgs, tabs(), map_ct() + hp_.plain_id(), step, pts, roots_g_, wrows, vrows,
                                 dhits, dfound, (u32)hstride, st_);
            } else {
                u64 *wrows = ws(n_occ * n);
                u64 cs = 1;
                for (u32 j = 0; j < cosets; j++) {
                    launch_roots_gather(poly, n, docc, dcounts, (u32)n_occ, cs, T, wrows, st_);
                    d_ntt(wrows, n_occ, map_ct() + hp_.plain_id(), 1, false, false);
                    launch_roots_scan(wrows, n, (u32)n_occ, pts, cs, T, j == 0, poly, docc, dcounts, dhits, dfound, (u32)hstride, st_);
                    cs = roots_mul(cs, roots_g_, t, T.r1);
                }
            }
            launch_roots_mult(poly, n, docc, dcounts, (u32)n_occ, T, dhits, dfound, dmult, (u32)hstride, st_);
            down(a.out[0], dhits, a.out_words[0]);
            down32(a.out[1], dfound, n_occ);
            down32(a.out[1] + n_occ, dmult, n_occ * hstride);
        } break;
        case STEP_ROOTS_SPLIT: {
            // polys = k, e0 = hstride; in[0] hits [n_occ][hstride], in[1] found [n_occ], in[2] mult [n_occ][hstride], in[3] counts [n] (the
            // occupied bins: 1 <= count, not LOOKUP_NONE, in slot order), in[4] part_stride [k] -> out[0] the parts' lists, part p at
            // n * (part_stride[0] + .. + part_stride[p - 1]) (in: poison), out[1] counts_out [k][n], the failure word
            const size_t k = polys, hstride = e0;
            need(k >= 1 && k < ROWS_MAX, "roots_split: k (polys) out of range");
            need(hstride >= 1 && split_capacity((u32)std::min<size_t>(hstride, SPLIT_CAP_LARGE + 1)) != 0, "roots_split: hstride (e0) outside 1 .. 8192: no instance holds the list");
            in_is(3, n, "roots_split: in[3] counts [n]");
            fits32(a.in[3], n, "roots_split: in[3]");
            std::vector<u64> occ;
            for (size_t s = 0; s < n; s++)
                if (a.in[3][s] != LOOKUP_NONE && a.in[3][s] >= 1) { need(a.in[3][s] <= hstride, "roots_split: a count exceeds hstride"); occ.push_back(s); }
            const size_t n_occ = occ.size();
            need(n_occ >= 1, "roots_split: no occupied bin");
            in_is(0, n_occ * hstride, "roots_split: in[0] hits [n_occ][hstride]");
            in_is(1, n_occ, "roots_split: in[1] found [n_occ]");
            in_is(2, n_occ * hstride, "roots_split: in[2] mult [n_occ][hstride]");
            in_is(4, k, "roots_split: in[4] part_stride [k]");
            fits32(a.in[1], n_occ, "roots_split: in[1]");
            fits32(a.in[2], n_occ * hstride, "roots_split: in[2]");
            fits32(a.in[4], k, "roots_split: in[4]");
            std::vector<u64> off(k + 1, 0);
            for (size_t p = 0; p < k; p++) { need(a.in[4][p] <= SPLIT_CAP_LARGE, "roots_split: a part_stride above 8192"); off[p + 1] = off[p] + n * a.in[4][p]; }
            for (size_t r = 0; r < n_occ; r++) {
                const u64 c = a.in[3][occ[r]], nf = a.in[1][r], read = std::min(nf, c);
                for (size_t i = 0; i < read; i++) need(a.in[0][r * hstride + i] < std::min<u64>(t, (u64)1 << 32), "roots_split: a value that is read is not below min(plain_modulus, 2^32)");
                if (nf < c)
                    for (size_t i = 0; i < read; i++) need(a.in[2][r * hstride + i] <= SPLIT_MULT_MAX, "roots_split: a multiplicity that is read exceeds SPLIT_MULT_MAX");
                for (size_t p = 0; p < k; p++)
                    need(split_cut((u32)c, (u32)k, (u32)p + 1) - split_cut((u32)c, (u32)k, (u32)p) <= a.in[4][p], "roots_split: a part_stride is below a bin's share of that part");
            }
            out_is(0, off[k], "roots_split: out[0] the parts' lists, n * part_stride[p] words each");
            out_is(1, k * n + 1, "roots_split: out[1] counts_out [k][n], failure");
            const u64 *dhits = up(a.in[0], a.in_words[0]);
            const u32 *dfound = up32(a.in[1], n_occ), *dmult = up32(a.in[2], n_occ * hstride), *dcounts = up32(a.in[3], n), *docc = up32(occ.data(), n_occ);
            const u32 *dstride = up32(a.in[4], k);
            const u64 *doff = up(off.data(), k);
            u64 *o = up(a.out[0], a.out_words[0]);
            u32 *dco = ws_as<u32>(k * n, 1);
            HIP_CHECK(hipMemsetAsync(dco, 0xee, k * n * sizeof(u32), st_));   // (the launcher zeroes them)
            u64 *fail = ws(1);
            HIP_CHECK(hipMemsetAsync(fail, 0xff, sizeof(u64), st_));
            sync();                                                    // (occ and off are this block's own)
            launch_roots_split(dhits, dfound, dmult, (u32)hstride, docc, dcounts, (u32)n_occ, (u32)k, o, doff, dstride, dco, (u32)n, fail, st_);
            down(a.out[0], o, a.out_words[0]);
            down32(a.out[1], dco, k * n);
            down(a.out[1] + k * n, fail, 1);
        } break;
        case STEP_ENTRIES_SCATTER: {
            // batch = locations, polys = F, terms = stride, e0 = k; bits per felt, item_bit_count and cap = max_items_per_bin - 1 are the
            // context's.  in[0] items [count][2] (count = offsets[batch] - offsets[0]; may be null when 0), in[1] offsets [batch + 1],
            // in[2] kstart [batch] -> out[0] roots [bins][stride] (in: what the words nobody writes keep; bins from its size), out[1] counts [n]
            const size_t locations = batch, F = polys, stride = terms, k = e0;
            need(has_psu_, "entries_scatter: the context was created without PSUParams");
            const u32 bpf = psu_.item_bit_count_per_felt, item_bits = psu_.item_bit_count, max_items = psu_.table_params.max_items_per_bin;
            need(max_items >= 2, "entries_scatter: max_items_per_bin < 2");
            need(locations >= 1 && F >= 1 && F <= SCATTER_MAX_F && (F - 1) * bpf < 128 && locations * F <= n, "entries_scatter: locations (batch) or F (polys) out of range");
            need(stride >= 1 && stride < ROWS_MAX && k < ROWS_MAX, "entries_scatter: stride (terms) or k (e0) out of range");
            in_is(1, locations + 1, "entries_scatter: in[1] offsets [locations + 1]");
            in_is(2, locations, "entries_scatter: in[2] kstart [locations]");
            fits32(a.in[2], locations, "entries_scatter: in[2]");
            need(a.out[0] && a.out_words[0] % stride == 0 && a.out_words[0] / stride >= locations * F && a.out_words[0] / stride <= n, "entries_scatter: out[0] roots [bins][stride], locations * F <= bins <= n");
            out_is(1, n, "entries_scatter: out[1] counts [n]");
            for (size_t l = 0; l < locations; l++) {
                need(a.in[1][l + 1] >= a.in[1][l] && a.in[1][l + 1] - a.in[1][l] <= 0xFFFFFFFFull, "entries_scatter: offsets decrease, or a location holds more than 2^32 - 1 entries");
                need(bulk_chunk((u32)a.in[2][l], (u32)(a.in[1][l + 1] - a.in[1][l]), (u32)k, max_items - 1).len <= stride, "entries_scatter: a location's chunk is longer than stride");
            }
            const size_t count = a.in[1][locations] - a.in[1][0];
            if (count) in_is(0, 2 * count, "entries_scatter: in[0] items [count][2]");
            const u64 *ditems = up(a.in[0], 2 * count), *doff = up(a.in[1], locations + 1);
            const u32 *dk = up32(a.in[2], locations);
            u64 *droots = up(a.out[0], a.out_words[0]);
            u32 *dc = ws_as<u32>(n, 1);
            HIP_CHECK(hipMemsetAsync(dc, 0xee, n * sizeof(u32), st_));  // (the kernel writes every one)
            launch_entries_scatter(ditems, doff, dk, (u32)locations, (u32)F, bpf, item_bits, max_items - 1, (u32)k, (u32)stride, droots, dc, (u32)n, 0, st_);
            down(a.out[0], droots, a.out_words[0]);
            down32(a.out[1], dc, n);
        } break;
        default: refuse("unknown step");
        }
        sync();
        for (auto &f : after) f();
    });
}

} // namespace apsu_he
