"""N1, the update: apsu_he_bundle_update on a full-degree 16M-4096 BinBundle (8190 bins x 1303 items) against apsu_he_db_build_bundle
of the same final bins -- one insert in each of 1, 64 and all bins, and 64 inserts + 64 removes.  Host wall time of the synchronous
calls (input copies included: the update sends the lists it is given, the build all roots), median of --reps after --warmup."""
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
t = ctx.t
bins = ctx.info.items_per_bundle * 5
D = ctx.max_items_per_bin - 1
rng = np.random.default_rng(1)
roots = np.zeros((bins, D + 1), dtype=np.uint64)                 # one spare column for the inserted item
roots[:, :D] = rng.integers(0, t, (bins, D), dtype=np.uint64)
u32 = lambda a: C.c_void_p(a.ctypes.data)


def build(counts):
    h = C.c_void_p()
    _check(L.apsu_he_db_build_bundle(ctx.h, 0, 0, _p(roots), u32(counts), bins, D + 1, C.byref(h)))
    return h


def update(old, ins, ins_counts, rem, rem_counts):
    h = C.c_void_p()
    _check(L.apsu_he_bundle_update(ctx.h, old, _p(ins) if ins is not None else None, u32(ins_counts) if ins is not None else None, 1,
                                   _p(rem) if rem is not None else None, u32(rem_counts) if rem is not None else None, 1, bins, C.byref(h)))
    return h


def median_ms(fn):
    times = []
    for rep in range(args.warmup + args.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        h = fn()
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        L.apsu_he_bundle_free(h)
        if rep >= args.warmup:
            times.append(dt * 1e3)
    return statistics.median(times), min(times), max(times)


full = np.full(bins, D, dtype=np.uint32)
old = build(full)
print(f"{args.params}: {bins} bins x {D} items, degree {D}; median (min .. max) of {args.reps} in ms")
print("  build_bundle, all bins as they are          : %.2f (%.2f .. %.2f)   [%.1f MB of roots sent]" % (*median_ms(lambda: build(full)), bins * (D + 1) * 8 / 1e6))
for k in (1, 64, bins):
    ins = rng.integers(0, t, (bins, 1), dtype=np.uint64)
    ic = np.zeros(bins, dtype=np.uint32); ic[:k] = 1
    roots[:, D] = ins[:, 0]
    after = full + ic
    print("  update_bundle, 1 insert in each of %4d bins : %.2f (%.2f .. %.2f)" % (k, *median_ms(lambda: update(old, ins, ic, None, None))))
    print("  build_bundle of those final bins             : %.2f (%.2f .. %.2f)" % median_ms(lambda: build(after)))
# 64 removes (bins 0 .. 63 lose their first item) and 64 inserts (bins 64 .. 127)
rem = np.ascontiguousarray(roots[:, :1]); rc = np.zeros(bins, dtype=np.uint32); rc[:64] = 1
ins = rng.integers(0, t, (bins, 1), dtype=np.uint64); ic = np.zeros(bins, dtype=np.uint32); ic[64:128] = 1
print("  update_bundle, 64 inserts + 64 removes       : %.2f (%.2f .. %.2f)" % median_ms(lambda: update(old, ins, ic, rem, rc)))
L.apsu_he_bundle_free(old)
