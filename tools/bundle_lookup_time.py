"""N1, find and place: apsu_he_bundle_bin_counts, apsu_he_bundles_lookup and apsu_he_db_apply_entries on a full-degree 16M-4096
BinBundle (8190 bins x 1303 items).  Host wall time of the synchronous calls (planning on the host and the copies included), and for
the lookups the device time of the decode and of the kernels behind it from the context's events (apsu_he_debug_lookup_times); the
same membership test on the host against the roots (numpy, one core) next to them.  Median of --reps after --warmup."""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, apsu_amd

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--params", default="16M-4096")
args = ap.parse_args()

ctx = apsu_amd.HeContext(open(os.path.join(ROOT, "tests", "params", args.params + ".json")).read())
t, F = ctx.t, ctx.felts_per_item
bins = ctx.info.items_per_bundle * F
D = ctx.max_items_per_bin - 1
rng = np.random.default_rng(1)
roots = rng.integers(0, t, (bins, D), dtype=np.uint64)
old = ctx.build_bundle(0, 0, [r for r in roots])


def entries(count):
    """half of them items that are in (part j taken from bin s + j), half random values"""
    start = (rng.integers(0, bins // F, count) * F).astype(np.uint32)
    felts = rng.integers(0, t, (count, F), dtype=np.uint64)
    inside = np.arange(count) % 2 == 0
    col = rng.integers(0, D, count)
    for j in range(F):
        felts[inside, j] = roots[start[inside] + j, col[inside]]
    return felts, start, inside


def median(fn, extra=None):
    wall, dec, ker = [], [], []
    for rep in range(args.warmup + args.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        if rep >= args.warmup:
            wall.append(dt * 1e3)
            a, k = ctx.lookup_times()
            dec.append(a); ker.append(k)
    return wall, dec, ker


fmt = lambda v: "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))
print(f"{args.params}: {bins} bins x {D} items, degree {D}, decoded array {(D + 1) * ctx.n * 8 / 1e6:.1f} MB; median (min .. max) of {args.reps} in ms")
wall, dec, ker = median(lambda: ctx.bin_counts(old))
print("  bin_counts                      : wall %s   decode %s   k_bin_counts + copy %s" % (fmt(wall), fmt(dec), fmt(ker)))
for count in (1, 4096, 100000):
    felts, start, inside = entries(count)
    present, room = ctx.lookup([old], (felts, start))
    assert (present[0] == inside).all() or count > 1000, "lookup disagrees with how the entries were made"
    wall, dec, ker = median(lambda: ctx.lookup([old], (felts, start)))
    kms = statistics.median(ker)
    print("  lookup of %6d entries        : wall %s   decode %s   k_bin_counts + k_bins_lookup + copies %s" % (count, fmt(wall), fmt(dec), fmt(ker)))
    print("      kernels against the decoded array's size: %.1f GB/s" % ((D + 1) * ctx.n * 8 / (kms * 1e-3) / 1e9))
    # the same test on the host against the roots: every part compared with the roots of its bin, in blocks of 2048 entries
    t0 = time.perf_counter()
    ok = np.ones(count, dtype=bool)
    for b0 in range(0, count, 2048):
        for j in range(F):
            ok[b0:b0 + 2048] &= (roots[start[b0:b0 + 2048] + j] == felts[b0:b0 + 2048, j:j + 1]).any(axis=1)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert (ok == present[0]).all()
    print("      host (numpy, one core, the roots at hand): %.2f ms" % host_ms)
felts, start, inside = entries(128)
rem = (np.ascontiguousarray(felts[0::2]), np.ascontiguousarray(start[0::2]))
ins = (np.ascontiguousarray(felts[1::2]), np.ascontiguousarray(start[1::2]))
res = ctx.apply_entries([old], inserts=ins, removes=rem)
print("  apply_entries, 64 inserts + 64 removes: states %s, %d removed, %d inserted, %d appended" % (
    list(res.state), int((res.rem_status == 2).sum()), int((res.ins_status == 0).sum()), len(res.appended)))
wall, _, _ = median(lambda: ctx.apply_entries([old], inserts=ins, removes=rem))
print("  apply_entries, 64 inserts + 64 removes: wall %s" % fmt(wall))
