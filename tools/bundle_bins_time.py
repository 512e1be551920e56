"""N1, reading the bins back: apsu_he_bundle_bins on full-degree BinBundles of 16M-4096 (8190 bins x 1303 items) and 256M-4096
(x 3999) and on a sparse one (64 occupied bins of 16M-4096).  Device time split by the context's events (apsu_he_debug_bins_times)
into decode + counts, the root search (k_bin_roots) and multiplicities + copy-back, next to the host wall time of the synchronous call
(the sort and the sum check on the host included) and the number of limb transforms the search does, bins x cosets.  The answer of the
first call is compared with the roots the BinBundle was built from.  Median of --reps after --warmup.

Every case runs in a child process of its own under a time limit, one after the other; the first that fails ends the run.
--composed also times the per-coset composition (gather + library transform + scan) once for the named case."""
import argparse, ctypes as C, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {                                   # name -> (parameter file, occupied bins or None for all, time limit of the child in s)
    "16M-full": ("16M-4096", None, 600),
    "16M-sparse": ("16M-4096", 64, 300),
    "256M-full": ("256M-4096", None, 900),
}

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--case", choices=sorted(CASES), help="run this case here (otherwise: every case of --cases in a child process)")
ap.add_argument("--cases", default="16M-full,16M-sparse,256M-full")
ap.add_argument("--composed", action="store_true", help="time the per-coset composition once as well")
args = ap.parse_args()

if not args.case:
    for name in args.cases.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps), "--warmup", str(args.warmup)]
        if args.composed and name == "16M-full":
            cmd.append("--composed")
        rc = subprocess.run(cmd, timeout=CASES[name][2]).returncode
        if rc != 0:
            sys.exit("case %s ended with status %d: stopping here" % (name, rc))
    sys.exit(0)

import numpy as np, apsu_amd
from apsu_amd import engine as E

params, occupied, _ = CASES[args.case]
ctx = apsu_amd.HeContext(open(os.path.join(ROOT, "tests", "params", params + ".json")).read())
t, n = ctx.t, ctx.n
bins = ctx.info.items_per_bundle * ctx.felts_per_item
D = ctx.max_items_per_bin - 1
rng = np.random.default_rng(1)
roots = rng.integers(0, t, (bins, D), dtype=np.uint64)          # uniform values: double roots come by themselves (about D^2 / 2t per bin)
if occupied is None:
    lists = [r for r in roots]
else:
    keep = set(int(v) for v in np.linspace(0, bins - 1, occupied).astype(int))
    lists = [roots[s] if s in keep else roots[s][:0] for s in range(bins)]
b = ctx.build_bundle(0, 0, lists)
want = [np.sort(x) for x in lists]
n_occ = sum(1 for x in lists if len(x))
cosets = (t - 1) // n
doubles = sum(len(x) - len(np.unique(x)) for x in lists)

lib = E.load_library()
counts = np.zeros(n, dtype=np.uint32)
out = np.zeros((n, D), dtype=np.uint64)


def call(form):
    t0 = time.perf_counter()
    E._check(lib.apsu_he_debug_bundle_bins_form(ctx.h, b.h, C.c_void_p(out.ctypes.data), C.c_void_p(counts.ctypes.data), C.c_uint32(D), C.c_int(form)))
    return (time.perf_counter() - t0) * 1e3, ctx.bins_times()


def check():
    assert [int(c) for c in counts[:bins]] == [len(x) for x in lists] and (counts[bins:] == E.NOT_A_BIN).all()
    assert all((out[s, :len(w)] == w).all() for s, w in enumerate(want)), "the bins read back differ from the roots"


fmt = lambda v: "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))
print(f"{args.case}: {params}, t = {t} ({t.bit_length()} bits), n = {n}, {n_occ} occupied bins x {D} items, {cosets} cosets, "
      f"{n_occ * cosets} limb transforms, {doubles} repeated values; median (min .. max) of {args.reps} in ms", flush=True)
wall, parts = [], []
for rep in range(args.warmup + args.reps):
    w, p = call(1)
    if rep == 0:
        check()
    if rep >= args.warmup:
        wall.append(w); parts.append(p)
search = statistics.median([p[1] for p in parts])
print("  wall %s   decode + counts %s   k_bin_roots %s   multiplicities + copy-back %s" % (
    fmt(wall), fmt([p[0] for p in parts]), fmt([p[1] for p in parts]), fmt([p[2] for p in parts])), flush=True)
print("  k_bin_roots: %.3f M limb transforms / s" % (n_occ * cosets / (search * 1e-3) / 1e6), flush=True)
if args.composed:
    w, p = call(2)
    check()
    print("  the per-coset composition, once: wall %.1f   search %.1f ms = %.3f M limb transforms / s" % (w, p[1], n_occ * cosets / (p[1] * 1e-3) / 1e6), flush=True)
