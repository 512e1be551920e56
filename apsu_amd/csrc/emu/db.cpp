// CPU emulation, the rows of a resident database (kernels_db.hip's headers): update, lookup, evaluation, merge, the bins' rows, and the
// host rules that place, compact and move them.  Each kernel's loop structure with an explicit loop over the lanes of its waves.
#include <algorithm>
#include <stdexcept>
#include <vector>

#include "emu_common.h"
#include "bin_eval.h"
#include "bin_lookup.h"
#include "bin_merge.h"
#include "bin_rows.h"
#include "bin_update.h"
#include "db_compact.h"
#include "db_place.h"
#include "db_rebase.h"
#include "multi_place.h"
#include "params.h"

using namespace apsu_he;

extern "C" {

// k_bins_update on one bin, as the wave runs it (bin_update.h): coefficient i in lane i % 64, register slot i / 64, every shuffle an
// explicit loop over the 64 lanes.  in / out: `rows` coefficients mod t (out may alias nothing; it is written on success only).
// Removals first, then insertions.  Returns the new count (index of the highest non-zero coefficient) or -1 with
// status[0] = 1: rem[status[1]] left a remainder; 2: the zero polynomial (not a bin); 3: the result needs more than `rows` coefficients.
int64_t emu_bin_update(uint64_t t_, const uint64_t *in, uint32_t rows, const uint64_t *rem, uint32_t n_rem, const uint64_t *ins, uint32_t n_ins,
                       uint64_t *out, int64_t *status)
{
    const ModulusInfo mi(t_);
    const Mod t{ t_, mi.ratio[0], mi.ratio[1] };
    constexpr int W = BIN_LANES;
    const int slots = (int)((rows + W - 1) / W);
    std::vector<std::vector<u64>> P(slots, std::vector<u64>(W, 0));
    int top = -1;
    for (int j = 0; j < slots; j++)
        for (int lane = 0; lane < W; lane++) {
            const u32 d = (u32)(j * W + lane);
            P[j][lane] = d < rows ? in[d] : 0;
            if (P[j][lane]) top = std::max(top, (int)d);          // the wave's max-reduction
        }
    status[0] = status[1] = 0;
    if (top < 0) { status[0] = 2; return -1; }
    u32 cnt = (u32)top;
    for (u32 r = 0; r < n_rem; r++) {
        const u64 a = rem[r];
        const int jmax = (int)(cnt >> 6);
        u64 carry = 0;
        for (int j = slots - 1; j >= 0; j--) {
            if (j > jmax) continue;
            std::vector<ScanPair> p(W);
            for (int lane = 0; lane < W; lane++) p[lane] = ScanPair{ a, P[j][lane] };
            for (int o = 1; o < W; o <<= 1) {
                std::vector<ScanPair> up(W);
                for (int lane = 0; lane < W; lane++) up[lane] = p[lane + o < W ? lane + o : lane];      // __shfl_down
                for (int lane = 0; lane < W; lane++) if (lane + o < W) p[lane] = bin_scan_compose(p[lane], up[lane], t);
            }
            std::vector<u64> sv(W);
            for (int lane = 0; lane < W; lane++) sv[lane] = bin_scan_carry(p[lane], carry, t);
            for (int lane = 0; lane < W; lane++) P[j][lane] = lane == W - 1 ? carry : sv[lane + 1];
            carry = sv[0];
        }
        if (carry != 0) { status[0] = 1; status[1] = r; return -1; }
        cnt--;
    }
    for (u32 r = 0; r < n_ins; r++) {
        if (cnt + 2 > rows) { status[0] = 3; return -1; }
        const u64 a = ins[r], neg_a = a ? t.q - a : 0;
        const int jmax = (int)((cnt + 1) >> 6);
        for (int j = slots - 1; j >= 0; j--) {
            if (j > jmax) continue;
            std::vector<u64> prev(W);
            for (int lane = 0; lane < W; lane++) prev[lane] = lane ? P[j][lane - 1] : (j > 0 ? P[j - 1][W - 1] : 0);
            for (int lane = 0; lane < W; lane++) P[j][lane] = bin_insert_step(P[j][lane], prev[lane], neg_a, t);
        }
        cnt++;
    }
    for (u32 d = 0; d < rows; d++) out[d] = P[d / W][d % W];
    return (int64_t)cnt;
}

uint64_t emu_bin_unlift(uint64_t x, uint64_t t, uint64_t q0) { return bin_unlift(x, t, q0); }

// k_bin_counts over poly[rows][n]: one lane per slot, rows walked from the top
void emu_bin_counts(const uint64_t *poly, uint64_t n, uint32_t rows, uint32_t *counts)
{
    for (size_t i = 0; i < n; i++) {
        int top = (int)rows - 1;
        while (top >= 0 && poly[(size_t)top * n + i] == 0) top--;
        counts[i] = bin_count_of(top);
    }
}

// k_bins_lookup<R> over poly[degree + 1][n] as the waves run it (bin_lookup.h): the points laid out by lookup_plan, one wave per work
// item, an explicit loop over its 64 lanes, R accumulators per lane, rows from the top four at a time.  flags[count * F] must come in
// as 0xEE: a part that no lane writes keeps it.  stats (may be null): work items, rows of point storage, largest nrows of a work item.
// Returns 0, or -1 (emu_last_error) for an entry that does not lie inside the n slots or an R outside 1 .. 16.
int emu_bins_lookup(uint64_t t_, const uint64_t *poly, uint64_t n, uint32_t degree, const uint64_t *felts, const uint32_t *start, uint64_t count,
                    uint32_t F, int R, unsigned char *flags, uint64_t *stats)
{
    return guarded([&]() -> int {
        if (R < 1 || R > 16) throw std::invalid_argument("R out of range");
        for (size_t e = 0; e < count; e++)
            if ((u64)start[e] + F > n) throw std::invalid_argument("entry beyond the last slot");
        const ModulusInfo mi(t_);
        const Mod t{ t_, mi.ratio[0], mi.ratio[1] };
        const LookupPlan plan = lookup_plan(felts, start, count, F, n, R);
        u32 widest = 0;
        for (const LookupWork &wk : plan.work) {
            widest = std::max(widest, wk.nrows);
            for (u32 lane = 0; lane < LOOKUP_LANES; lane++) {
                const size_t slot = (size_t)wk.tile * LOOKUP_LANES + lane;
                const bool live = slot < n;
                const u64 *col = poly + (live ? slot : 0);
                u64 x[16], acc[16];
                for (int r = 0; r < R; r++) {
                    x[r] = (u32)r < wk.nrows ? plan.pts[((size_t)wk.row0 + r) * LOOKUP_LANES + lane] : 0;
                    acc[r] = 0;
                }
                u64 nz = 0;
                int d = (int)degree;
                for (; d >= 3; d -= 4) {
                    u64 p[4];
                    for (int k = 0; k < 4; k++) p[k] = col[(size_t)(d - k) * n];
                    for (int k = 0; k < 4; k++) {
                        nz |= p[k];
                        for (int r = 0; r < R; r++) acc[r] = lookup_horner_step(acc[r], x[r], p[k], t);
                    }
                }
                for (; d >= 0; d--) {
                    const u64 p = col[(size_t)d * n];
                    nz |= p;
                    for (int r = 0; r < R; r++) acc[r] = lookup_horner_step(acc[r], x[r], p, t);
                }
                for (int r = 0; r < R && (u32)r < wk.nrows; r++) {
                    const u32 part = plan.idx[((size_t)wk.row0 + r) * LOOKUP_LANES + lane];
                    if (part != LOOKUP_NONE) flags[part] = live && lookup_found(acc[r], nz) ? 1 : 0;
                }
            }
        }
        if (stats) { stats[0] = plan.work.size(); stats[1] = plan.rows(); stats[2] = widest; }
        return 0;
    });
}

// k_bins_eval over poly[rows][n] as the waves run it (bin_eval.h): one wave per tile of 64 slots, the tile's top from the counts of
// emu_bin_counts, an explicit loop over its 64 lanes, rows from the top EVAL_ROWS at a time.  mask, is_bin and walked may be null;
// out[n] and is_bin[n] must come in as 0xEE bytes (a word that no lane writes keeps them); walked[tiles] = the rows a tile read.
// wide: 0 = the width the launch takes for t, 1 = the 128-bit step whatever t (both must agree wherever both are exact).
// Returns 0, or -1 (emu_last_error) for a value that is not below t.
int emu_bins_eval(uint64_t t_, const uint64_t *poly, uint64_t n, uint32_t rows, const uint64_t *x, const uint64_t *mask, int wide, uint64_t *out,
                  unsigned char *is_bin, uint32_t *walked)
{
    return guarded([&]() -> int {
        for (size_t s = 0; s < n; s++)
            if (x[s] >= t_ || (mask && mask[s] >= t_)) throw std::invalid_argument("slot value is not reduced modulo the plain modulus");
        const ModulusInfo mi(t_);
        const Mod t{ t_, mi.ratio[0], mi.ratio[1] };
        const bool narrow = !wide && merge_narrow(merge_bits(t_));
        std::vector<u32> counts(n);
        emu_bin_counts(poly, n, rows, counts.data());
        const size_t tiles = (n + EVAL_LANES - 1) / EVAL_LANES;
        for (size_t tile = 0; tile < tiles; tile++) {
            int top = -1;
            for (int lane = 0; lane < EVAL_LANES; lane++) {
                const size_t slot = tile * EVAL_LANES + lane;
                top = std::max(top, eval_count_top(slot < n ? counts[slot] : LOOKUP_NONE));
            }
            const int d0 = eval_walk_top(top, rows);
            if (walked) walked[tile] = (uint32_t)(d0 + 1);
            for (int lane = 0; lane < EVAL_LANES; lane++) {
                const size_t slot = tile * EVAL_LANES + lane;
                if (slot >= n) continue;
                const u64 *col = poly + slot;
                const u64 xs = x[slot];
                const u64 acc = narrow ? eval_walk<true>(col, n, d0, xs, t) : eval_walk<false>(col, n, d0, xs, t);
                out[slot] = eval_finish(acc, mask ? mask[slot] : 0, t);
                if (is_bin) is_bin[slot] = eval_is_bin(counts[slot]) ? 1 : 0;
            }
        }
        return 0;
    });
}
int emu_eval_rows() { return EVAL_ROWS; }

// self_test_reduce over `count` reports (bin_eval.h), each sizeof(SelfTestReport) bytes; emu_self_test_report_bytes gives the size
int emu_self_test_report_bytes() { return (int)sizeof(SelfTestReport); }
void emu_self_test_reduce(const void *parts, int count, void *out)
{
    SelfTestReport r = self_test_empty();
    for (int i = 0; i < count; i++) self_test_reduce(r, static_cast<const SelfTestReport *>(parts)[i]);
    *static_cast<SelfTestReport *>(out) = r;
}

// rebase_compatible of two parameter files: 1 compatible, 0 not (the reason in emu_last_error), -1 a file that does not load
int emu_rebase_compatible(const char *src_json, const char *dst_json)
{
    return guarded([&]() -> int {
        const std::string why = rebase_compatible(PSUParams::Load(src_json), PSUParams::Load(dst_json));
        g_err = why;
        return why.empty() ? 1 : 0;
    });
}

// rebase_plan: parts [n_bundles], first [n_bundles]; cache_idx / origin [capacity].  Returns the number of output BinBundles, -1 on a
// refusal, -2 when capacity is too small.
int64_t emu_rebase_plan(const uint32_t *max_count, const uint32_t *bundle_idx, uint32_t n_bundles, uint32_t dst_max_items, uint32_t *parts, uint32_t *first,
                        uint32_t *cache_idx, uint32_t *origin, uint64_t capacity)
{
    return guarded([&]() -> int64_t {
        const RebasePlan plan = rebase_plan(max_count, bundle_idx, n_bundles, dst_max_items);
        if (plan.cache_idx.size() > capacity) return -2;
        std::copy(plan.parts.begin(), plan.parts.end(), parts);
        std::copy(plan.first.begin(), plan.first.end(), first);
        std::copy(plan.cache_idx.begin(), plan.cache_idx.end(), cache_idx);
        std::copy(plan.origin.begin(), plan.origin.end(), origin);
        return (int64_t)plan.cache_idx.size();
    });
}

// place_entries (db_place.h).  counts [n_bundles][bins]; *_present [n_bundles][count]; felts [count][F].  Outputs: per entry status and
// target; state [n_bundles]; *n_new; the per-bin lists of every BinBundle, given and appended, in apsu_he_bundle_update's layout with the
// caller's stride: *_counts_out [n_bundles + n_ins][bins], *_roots_out [n_bundles + n_ins][bins][stride] (rows beyond n_bundles + *n_new
// are not written).  Returns 0; -1: a refusal (std::invalid_argument); -2: a list longer than `stride`.  Text: emu_last_error.
int emu_place_entries(uint32_t n_bundles, uint32_t bins, uint32_t F, uint64_t t, uint32_t max_items, const uint32_t *counts,
                      const unsigned char *ins_present, const unsigned char *rem_present, const uint64_t *ins_felts, const uint32_t *ins_start,
                      uint64_t n_ins, const uint64_t *rem_felts, const uint32_t *rem_start, uint64_t n_rem, uint32_t *ins_status, uint32_t *ins_target,
                      uint32_t *rem_status, uint32_t *rem_target, uint32_t *state, uint32_t *n_new, uint32_t stride, uint32_t *ins_counts_out,
                      uint64_t *ins_roots_out, uint32_t *rem_counts_out, uint64_t *rem_roots_out)
{
    try {
        PlaceInput in;
        in.n_bundles = n_bundles; in.bins = bins; in.F = F; in.max_items = max_items; in.t = t;
        in.counts = counts; in.ins_present = ins_present; in.rem_present = rem_present;
        in.ins_felts = ins_felts; in.ins_start = ins_start; in.n_ins = n_ins;
        in.rem_felts = rem_felts; in.rem_start = rem_start; in.n_rem = n_rem;
        const PlaceResult out = place_entries(in);
        std::copy(out.ins_status.begin(), out.ins_status.end(), ins_status);
        std::copy(out.ins_target.begin(), out.ins_target.end(), ins_target);
        std::copy(out.rem_status.begin(), out.rem_status.end(), rem_status);
        std::copy(out.rem_target.begin(), out.rem_target.end(), rem_target);
        std::copy(out.state.begin(), out.state.end(), state);
        *n_new = out.n_new;
        for (int kind = 0; kind < 2; kind++)
            for (size_t b = 0; b < out.ins.size(); b++) {
                const PlaceLists &l = kind ? out.rem[b] : out.ins[b];
                uint32_t *co = (kind ? rem_counts_out : ins_counts_out) + b * bins;
                uint64_t *ro = (kind ? rem_roots_out : ins_roots_out) + b * bins * (size_t)stride;
                if (l.stride > stride) { g_err = "list longer than stride"; return -2; }
                for (u32 s = 0; s < bins; s++) {
                    co[s] = l.any() ? l.counts[s] : 0;
                    for (u32 r = 0; r < co[s]; r++) ro[(size_t)s * stride + r] = l.roots[(size_t)s * l.stride + r];
                }
            }
        return 0;
    } catch (const std::invalid_argument &e) { g_err = e.what(); return -1;
    } catch (const std::exception &e) { g_err = e.what(); return -3; }
}

// k_bins_merge over A[dA + 1][n] and B[dB + 1][n] as the waves run it (bin_merge.h): one wave per (tile, block of K output rows), an explicit
// loop over its 64 lanes, the K-row window of B in slots r mod K, the walk in chunks of K steps from a multiple of K, a fold every
// `fold` steps (0: merge_fold_interval(bits(t)), the device's; the sums are 64-bit for t < 2^32 and 128-bit otherwise, as there).
// The tops come from emu_bin_counts of each input, the refusals from merge_counts without a bound on the sum.  C: [dA + dB + 1][n].
// stats (may be null): work items, folds inside the walks, longest walk in steps.  Returns 0, or -1 (emu_last_error).
int emu_bins_merge(uint64_t t_, const uint64_t *A, uint32_t dA, const uint64_t *B, uint32_t dB, uint64_t n, int K, uint32_t fold, uint64_t *C,
                   uint64_t *stats)
{
    return guarded([&]() -> int {
        if (K < 1 || K > 16) throw std::invalid_argument("K out of range");
        const ModulusInfo mi(t_);
        const Mod t{ t_, mi.ratio[0], mi.ratio[1] };
        const int bits = merge_bits(t_);
        const bool narrow = merge_narrow(bits);
        if (!fold) fold = merge_fold_interval(bits);
        std::vector<u32> ca(n), cb(n), sum(n);
        emu_bin_counts(A, n, dA + 1, ca.data());
        emu_bin_counts(B, n, dB + 1, cb.data());
        merge_counts(ca.data(), cb.data(), n, 0, sum.data());
        const std::vector<int> topsA = merge_tile_tops(ca.data(), n), topsB = merge_tile_tops(cb.data(), n);
        const u32 rows = dA + dB + 1, blocks = (rows + K - 1) / K;
        u64 folds = 0, longest = 0;
        for (size_t tile = 0; tile < topsA.size(); tile++)
            for (u32 blk = 0; blk < blocks; blk++) {
                const int k0 = (int)blk * K, topA = topsA[tile], topB = topsB[tile];
                const MergeWalk wk = merge_walk(k0, K, topA, topB);
                if (wk.i1 >= wk.i0) longest = std::max(longest, (u64)((wk.i1 - wk.i0) / K + 1) * K);
                for (int lane = 0; lane < MERGE_LANES; lane++) {
                    const size_t slot = tile * MERGE_LANES + lane;
                    if (slot >= n) continue;                       // (the kernel's idle lanes work on slot 0 and store nothing)
                    const u64 *colA = A + slot, *colB = B + slot;
                    u64 acc64[16] = { 0 };
                    u128p acc128[16] = {};
                    if (wk.i1 >= wk.i0) {
                        auto rowB = [&](int r) -> u64 {
                            const int rc = r < 0 ? 0 : (r > topB ? topB : r);
                            const u64 v = colB[(size_t)rc * n];
                            return r == rc ? v : 0;
                        };
                        auto rowA = [&](int i) -> u64 {
                            const u64 v = colA[(size_t)(i > wk.i1 ? wk.i1 : i) * n];
                            return i <= wk.i1 ? v : 0;
                        };
                        u64 win[16];
                        win[0] = 0;
                        for (int j = 1; j < K; j++) win[j] = rowB(k0 - wk.i0 + j);
                        u32 pending = 0;
                        for (int ib = wk.i0; ib <= wk.i1; ib += K) {
                            u64 a[16], nb[16];
                            for (int u = 0; u < K; u++) {
                                a[u] = rowA(ib + u);
                                nb[u] = rowB(k0 - ib - u);
                            }
                            for (int u = 0; u < K; u++) {
                                if (pending == fold) {
                                    for (int j = 0; j < K; j++) {
                                        if (narrow) acc64[j] = merge_fold_narrow(acc64[j], t);
                                        else acc128[j] = u128p{ merge_fold_wide(acc128[j], t), 0 };
                                    }
                                    pending = 0;
                                    if (!lane) folds++;
                                }
                                pending++;
                                win[(K - u) % K] = nb[u];
                                for (int j = 0; j < K; j++) {
                                    if (narrow) merge_mac_narrow(acc64[j], a[u], win[(j - u + K) % K]);
                                    else merge_mac_wide(acc128[j], a[u], win[(j - u + K) % K]);
                                }
                            }
                        }
                    }
                    for (int j = 0; j < K && (u32)(k0 + j) < rows; j++)
                        C[(size_t)(k0 + j) * n + slot] = narrow ? merge_fold_narrow(acc64[j], t) : merge_fold_wide(acc128[j], t);
                }
            }
        if (stats) { stats[0] = topsA.size() * (u64)blocks; stats[1] = folds; stats[2] = longest; }
        return 0;
    });
}

uint32_t emu_merge_fold_interval(int bits) { return merge_fold_interval(bits); }
int emu_merge_fold_exact(int bits) { return merge_fold_exact(bits) ? 1 : 0; }
int emu_merge_k() { return MERGE_K; }

// merge_counts (bin_merge.h): sum[n], or -1 with the first offending slot named in emu_last_error.  max_items 0: no bound on the sum.
int emu_merge_counts(const uint32_t *a, const uint32_t *b, uint64_t n, uint32_t max_items, uint32_t *sum)
{
    return guarded([&]() -> int { merge_counts(a, b, n, max_items, sum); return 0; });
}

// merge_steps (bin_merge.h): rows[n_bundles - 1], tops[2 (n_bundles - 1) tiles], *degree.  Returns 0, -1 for merge_counts' refusals
// (std::invalid_argument) or -3 for the logic error, the text in emu_last_error.
int emu_merge_steps(const uint32_t *counts, const uint32_t *degrees, uint32_t n_bundles, uint64_t n, uint32_t max_items, uint32_t *rows, int *tops,
                    uint32_t *degree)
{
    try {
        if (!n_bundles) throw std::invalid_argument("no BinBundle");
        const MergeSteps ms = merge_steps(counts, degrees, n_bundles, n, max_items);
        std::copy(ms.rows.begin(), ms.rows.end(), rows);
        std::copy(ms.tops.begin(), ms.tops.end(), tops);
        *degree = ms.degree;
        return 0;
    } catch (const std::invalid_argument &e) { g_err = e.what(); return -1;
    } catch (const std::exception &e) { g_err = e.what(); return -3; }
}

// k_bins_rows over poly[rows][n] as the workgroups run it (bin_rows.h): one workgroup per tile of 64 slots x 64 degrees, an explicit
// loop over its waves and their 64 lanes, the padded LDS tile between the two phases.  counts: n words (emu_bin_counts' form);
// out: at least off[bins] words, where off is rows_offsets' scan, also returned in off_out (bins + 1 words, may be null).
// Returns off[bins], or -1 (emu_last_error).
int64_t emu_bins_rows(const uint64_t *poly, uint64_t n, uint32_t rows, const uint32_t *counts, uint32_t bins, uint64_t *off_out, uint64_t *out)
{
    return guarded([&]() -> int64_t {
        if (bins > n) throw std::invalid_argument("more bins than slots");
        const std::vector<u64> off = rows_offsets(counts, bins, rows);
        const std::vector<int> tops = rows_tile_tops(counts, n, bins);
        if (off_out) std::copy(off.begin(), off.end(), off_out);
        const u32 dtiles = (rows + ROWS_TILE - 1) / ROWS_TILE;
        std::vector<u64> tile(ROWS_LDS_WORDS);
        for (size_t bx = 0; bx < tops.size(); bx++)
            for (u32 by = 0; by < dtiles; by++) {
                const size_t s0 = bx * ROWS_TILE;
                const u32 d0 = by * ROWS_TILE;
                const int top = tops[bx];
                if ((int)d0 > top) continue;
                std::fill(tile.begin(), tile.end(), ~(u64)0);      // (what a live store reads was loaded: anything else would show)
                for (int wave = 0; wave < ROWS_WAVES; wave++)
                    for (int dl = wave; dl < ROWS_TILE; dl += ROWS_WAVES)
                        for (int lane = 0; lane < ROWS_TILE; lane++)
                            if (rows_load_live(d0 + dl, s0 + lane, rows, n, top)) tile[rows_lds_at(dl, lane)] = poly[(size_t)(d0 + dl) * n + s0 + lane];
                for (int wave = 0; wave < ROWS_WAVES; wave++)
                    for (int sl = wave; sl < ROWS_TILE; sl += ROWS_WAVES) {
                        const size_t s = s0 + sl;
                        if (s >= bins) break;
                        for (int lane = 0; lane < ROWS_TILE; lane++)
                            if (rows_store_live(d0 + lane, s, counts[s], bins)) out[off[s] + d0 + lane] = tile[rows_lds_at(lane, sl)];
                    }
            }
        return (int64_t)off[bins];
    });
}

// plan_compaction (db_compact.h).  counts [n_bundles][n]; group [n_bundles]; degree [n_bundles] (the first `return value` are written).
// Returns the number of groups.
int emu_plan_compaction(const uint32_t *counts, uint32_t n_bundles, uint64_t n, uint32_t max_items, uint32_t *group, uint32_t *degree)
{
    return guarded([&]() -> int {
        const CompactPlan plan = plan_compaction(counts, n_bundles, n, max_items);
        std::copy(plan.group.begin(), plan.group.end(), group);
        std::copy(plan.degree.begin(), plan.degree.end(), degree);
        return (int)plan.degree.size();
    });
}

// ---- the multi-device handle's rules (multi_place.h)
// place_new_unit: the slot, or -1 (emu_last_error)
int emu_place_new_unit(uint32_t bundle_idx, uint32_t bundle_idx_count, int world, const uint64_t *load)
{
    return guarded([&]() -> int { return place_new_unit(bundle_idx, bundle_idx_count, world, load); });
}

static std::vector<RegUnit> emu_units(const int32_t *slot, const uint32_t *bundle_idx, const uint32_t *cache_idx, const uint32_t *degree, uint32_t count)
{
    std::vector<RegUnit> v(count);
    for (uint32_t i = 0; i < count; i++) { v[i].slot = slot[i]; v[i].bundle_idx = bundle_idx[i]; v[i].cache_idx = cache_idx[i]; v[i].degree = degree[i]; }
    return v;
}

// device_loads: load[world]; 0, or -1
int emu_device_loads(const int32_t *slot, const uint32_t *degree, uint32_t count, int world, uint64_t *load)
{
    return guarded([&]() -> int {
        std::vector<uint32_t> zero(count, 0);
        const std::vector<uint64_t> l = device_loads(emu_units(slot, zero.data(), zero.data(), degree, count), world);
        std::copy(l.begin(), l.end(), load);
        return 0;
    });
}

// index_in_cache_order: ids[count] (the first `return value` are written), or -1: two BinBundles of the index share a cache_idx
int emu_index_in_cache_order(const uint32_t *bundle_idx, const uint32_t *cache_idx, uint32_t count, uint32_t which, int32_t *ids)
{
    return guarded([&]() -> int {
        std::vector<int32_t> slot(count, 0);
        std::vector<uint32_t> zero(count, 0);
        const std::vector<int> v = index_in_cache_order(emu_units(slot.data(), bundle_idx, cache_idx, zero.data(), count), which);
        std::copy(v.begin(), v.end(), ids);
        return (int)v.size();
    });
}

// merge_home of the members given by slot and cache_idx: the slot; *first = the position of the first member in cache order.  -1: no members
int emu_merge_home(const int32_t *slot, const uint32_t *cache_idx, uint32_t count, uint32_t *first)
{
    return guarded([&]() -> int {
        std::vector<uint32_t> zero(count, 0);
        const std::vector<RegUnit> m = emu_units(slot, zero.data(), cache_idx, zero.data(), count);
        if (first) *first = (uint32_t)merge_first(m);
        return merge_home(m);
    });
}

// registry_after.  The old registry and the appended BinBundles as four arrays each; dropped[old_count]; replaced_degree[old_count]
// (< 0: unchanged).  Outputs: new_id[old_count + n_appended] and the new registry's four arrays (capacity old_count + n_appended).
// Returns the new count, or -1 (emu_last_error).
int emu_registry_after(const int32_t *slot, const uint32_t *bundle_idx, const uint32_t *cache_idx, const uint32_t *degree, uint32_t old_count,
                       const unsigned char *dropped, const int64_t *replaced_degree, const int32_t *app_slot, const uint32_t *app_bundle_idx,
                       const uint32_t *app_cache_idx, const uint32_t *app_degree, uint32_t n_appended, int32_t *new_id, int32_t *out_slot,
                       uint32_t *out_bundle_idx, uint32_t *out_cache_idx, uint32_t *out_degree)
{
    return guarded([&]() -> int {
        const RegistryAfter r = registry_after(emu_units(slot, bundle_idx, cache_idx, degree, old_count),
                                               std::vector<unsigned char>(dropped, dropped + old_count),
                                               std::vector<int64_t>(replaced_degree, replaced_degree + old_count),
                                               emu_units(app_slot, app_bundle_idx, app_cache_idx, app_degree, n_appended));
        std::copy(r.new_id.begin(), r.new_id.end(), new_id);
        for (size_t i = 0; i < r.registry.size(); i++) {
            out_slot[i] = r.registry[i].slot; out_bundle_idx[i] = r.registry[i].bundle_idx;
            out_cache_idx[i] = r.registry[i].cache_idx; out_degree[i] = r.registry[i].degree;
        }
        return (int)r.registry.size();
    });
}

} // extern "C"
