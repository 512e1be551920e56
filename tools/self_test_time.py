"""Checking a resident database against plaintext: apsu_he_db_self_test on one full-degree BinBundle of 16M-4096 (8190 bins x 1303
items, built from items) and on the benchmark's database of that set (4 bundle indices x 7 BinBundles, degrees 6 x 1303 + 170, the
synthetic BinBundles of bench.py).  Device time split by the context's events (apsu_he_debug_self_test_times) into the decode, the
counts, k_bins_eval, the comparison and the homomorphic part (key generation to decryption), next to the host wall time of the
synchronous call; k_bins_eval's rate over the decoded arrays in bytes per second.  The first call's report must be clean.  Median of
--reps after --warmup.

Every case runs in a child process of its own under a time limit, one after the other; the first that fails ends the run."""
import argparse, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"one": 300, "db28": 600}           # name -> time limit of the child in s
PARAMS = "16M-4096"
SEED = bytes((13 * i + 5) & 0xFF for i in range(64))
SEED0 = 0x41505355                          # bench.py's database seeds

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--case", choices=sorted(CASES), help="run this case here (otherwise: every case of --cases in a child process)")
ap.add_argument("--cases", default="one,db28")
args = ap.parse_args()

if not args.case:
    for name in args.cases.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps), "--warmup", str(args.warmup)]
        rc = subprocess.run(cmd, timeout=CASES[name]).returncode
        if rc != 0:
            sys.exit("case %s ended with status %d: stopping here" % (name, rc))
    sys.exit(0)

import numpy as np, apsu_amd

ctx = apsu_amd.HeContext(open(os.path.join(ROOT, "tests", "params", PARAMS + ".json")).read())
t, n = ctx.t, ctx.n
D = ctx.max_items_per_bin - 1
if args.case == "one":
    bins = ctx.info.items_per_bundle * ctx.felts_per_item
    roots = np.random.default_rng(1).integers(0, t, (bins, D), dtype=np.uint64)
    bundles = [ctx.build_bundle(0, 0, [r for r in roots])]
    what = "one BinBundle built from items, %d bins x %d" % (bins, D)
else:
    degrees = [D] * 6 + [170]
    bundles = [ctx.random_bundle(b, ci, deg, SEED0 + 1000003 * b + 7919 * ci) for b in range(ctx.bundle_idx_count) for ci, deg in enumerate(degrees)]
    what = "%d bundle indices x %d synthetic BinBundles, degrees %s" % (ctx.bundle_idx_count, len(degrees), sorted(set(degrees), reverse=True))
decoded = sum((b.degree + 1) * n * 8 for b in bundles)

fmt = lambda v: "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))
print(f"{args.case}: {PARAMS}, t = {t} ({t.bit_length()} bits), n = {n}, {what}; decoded arrays {decoded / 2**20:.1f} MiB; "
      f"median (min .. max) of {args.reps} after {args.warmup} warm-up, ms", flush=True)
wall, parts, he, plain = [], [], [], []
for rep in range(args.warmup + args.reps):
    t0 = time.perf_counter()
    r = ctx.self_test(bundles, SEED)
    w = (time.perf_counter() - t0) * 1e3
    if rep == 0:
        print("  report:", r, flush=True)
        assert r.bundles == len(bundles) and r.slots == len(bundles) * n and r.mismatches == 0 and r.first_mismatch is None and r.min_budget > 0
    if rep >= args.warmup:
        wall.append(w); parts.append(ctx.self_test_times()); he.append(r.he_ms); plain.append(r.plain_ms)
names = ("decode", "k_bin_counts", "k_bins_eval", "comparison", "homomorphic part (keygen .. decrypt)")
print("  wall %s" % fmt(wall), flush=True)
for i, nm in enumerate(names):
    print("    %-40s %s" % (nm, fmt([p[i] for p in parts])), flush=True)
print("    %-40s %s" % ("plain part (decode .. comparison)", fmt(plain)), flush=True)
ev = statistics.median([p[2] for p in parts])
print("  k_bins_eval: %.1f GB/s over the decoded arrays (%d bytes in %.3f ms)" % (decoded / (ev * 1e-3) / 1e9, decoded, ev), flush=True)
