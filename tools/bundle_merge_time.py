"""N1, compaction: apsu_he_bundles_merge of two half-full full-width BinBundles (every bin of both holds (max_items_per_bin - 1) // 2
items) against apsu_he_db_build_bundle of the union; the merge's device time split into decode, product kernel and re-encode
(apsu_he_debug_merge_times); and one eval_bundles over the two BinBundles against one over the merged one (random source
ciphertexts and keys: times only).  Host wall time of the synchronous calls, median of --reps after --warmup."""
import argparse, ctypes as C, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, apsu_amd
from apsu_amd.engine import load_library, _check, _p

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--params", default="16M-4096")
args = ap.parse_args()

ctx = apsu_amd.HeContext(open(os.path.join(ROOT, "tests", "params", args.params + ".json")).read())
L = load_library()
n, t, K = ctx.n, ctx.t, ctx.K
bins = ctx.info.items_per_bundle * ctx.felts_per_item
H = (ctx.max_items_per_bin - 1) // 2
rng = np.random.default_rng(1)
roots = rng.integers(0, t, (bins, 2 * H), dtype=np.uint64)          # columns 0 .. H-1: A's items, H .. 2H-1: B's
u32 = lambda a: C.c_void_p(a.ctypes.data)


def build(r, count, cache_idx=0):
    h = C.c_void_p()
    r, counts = np.ascontiguousarray(r), np.full(bins, count, dtype=np.uint32)
    _check(L.apsu_he_db_build_bundle(ctx.h, 0, cache_idx, _p(r), u32(counts), bins, r.shape[1], C.byref(h)))
    return h


def merge(hs):
    h = C.c_void_p()
    _check(L.apsu_he_bundles_merge(ctx.h, (C.c_void_p * len(hs))(*hs), len(hs), 0, C.byref(h)))
    return h


def median_ms(fn, free=True, extra=None):
    times, rows = [], []
    for rep in range(args.warmup + args.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        h = fn()
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        if free:
            L.apsu_he_bundle_free(h)
        if rep >= args.warmup:
            times.append(dt * 1e3)
            if extra:
                rows.append(extra())
    return (statistics.median(times), min(times), max(times)), rows


a, b = build(roots[:, :H], H, 0), build(roots[:, H:], H, 1)
print(f"{args.params}: {bins} bins, two BinBundles of {H} items per bin -> one of {2 * H}; median (min .. max) of {args.reps} in ms")
print("  build_bundle of the union                    : %.2f (%.2f .. %.2f)   [%.1f MB of roots sent]" % (*median_ms(lambda: build(roots, 2 * H))[0], roots.nbytes / 1e6))
wall, split = median_ms(lambda: merge([a, b]), extra=ctx.merge_times)
print("  bundles_merge of the two                     : %.2f (%.2f .. %.2f)" % wall)
print("    device time by events: decode + counts %.3f, k_bins_merge %.3f, re-encode %.3f (medians)" % tuple(statistics.median(r[i] for r in split) for i in range(3)))
m = merge([a, b])

# one query's eval_bundles over the two BinBundles and over the merged one
first = ctx.first_chain_idx
Lf, ns = first + 1, ctx.source_power_count
src = np.stack([np.stack([np.stack([rng.integers(0, q, n, dtype=np.uint64) for q in ctx.q[:Lf]]) for _ in range(2)]) for _ in range(ns)])
rk = ctx.upload_relin_keys(np.stack([np.stack([np.stack([rng.integers(0, q, n, dtype=np.uint64) for q in ctx.q]) for _ in range(2)]) for _ in range(K - 1)]))
sd = torch.from_numpy(src.view(np.int64)).cuda()
pw = ctx.compute_powers([0], [[sd.data_ptr() + (s * 2 * Lf * n) * 8 for s in range(ns)]], rk, on_device=True)
md = torch.from_numpy(rng.integers(0, t, (2, n), dtype=np.uint64).view(np.int64)).cuda()
out = torch.zeros((2, 2, n), dtype=torch.int64, device="cuda")
wrap = lambda h, ci, deg: apsu_amd.Bundle(ctx, h, 0, ci, deg)
two, one = [wrap(a, 0, H), wrap(b, 1, H)], [wrap(m, 0, 2 * H)]
for name, bl in (("the two BinBundles", two), ("the merged BinBundle", one)):
    mp = [md.data_ptr() + i * n * 8 for i in range(len(bl))]
    f = lambda: ctx.eval_bundles(bl, pw, rk, mp, out=out.data_ptr(), masks_on_device=True, out_on_device=True)
    print("  eval_bundles over %-26s : %.3f (%.3f .. %.3f)" % ((name,) + median_ms(f, free=False)[0]))
