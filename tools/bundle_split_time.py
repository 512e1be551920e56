"""N1, splitting and moving: apsu_he_bundle_split and apsu_he_bundle_adopt on one full-degree BinBundle of 16M-4096 (8190 bins x 1303
items), next to the path that existed before them, measured in the same run: apsu_he_bundle_bins -> the roots on the host -> one
apsu_he_db_build_bundle per part in the other context.
  split   into 2 in the same context: host wall time of the synchronous call and the device spans of apsu_he_debug_split_times
          (decode + counts, root search + multiplicities, k_roots_split, the two builds)
  adopt   into a context that differs in ps_low_degree (and the query powers that go with it): wall time
  before  bins + host slicing + build_bundle per part (2 parts in the same context; 1 part in the other context)
The parts of the first split are compared with the builds of the sliced roots (images byte for byte), the adopted BinBundle with the
other context's build.  Median (min .. max) of --reps after --warmup, written to --out (default: the next free profiles/rNN_bundle_split.txt)."""
import argparse, ctypes as C, glob, json, os, re, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--params", default="16M-4096")
ap.add_argument("--out", default=None)
args = ap.parse_args()

import numpy as np, apsu_amd
from apsu_amd import engine as E

if args.out is None:
    taken = [int(m.group(1)) for m in (re.match(r"r(\d+)_", os.path.basename(p)) for p in glob.glob(os.path.join(ROOT, "profiles", "r*_*"))) if m]
    args.out = os.path.join(ROOT, "profiles", "r%02d_bundle_split.txt" % (max(taken + [0]) + 1))

js = open(os.path.join(ROOT, "tests", "params", args.params + ".json")).read()
other = json.loads(js)
other["query_params"]["ps_low_degree"] = 4                   # 16M-4096 has 44 with the sources 1, 3, 11, 18, 45, 225
other["query_params"]["query_powers"] = [1, 3, 5, 15, 45, 225]
src, dst = apsu_amd.HeContext(js), apsu_amd.HeContext(json.dumps(other))
t, n = src.t, src.n
bins = src.info.items_per_bundle * src.felts_per_item
D = src.max_items_per_bin - 1
rng = np.random.default_rng(1)
roots = np.sort(rng.integers(0, t, (bins, D), dtype=np.uint64), axis=1)      # uniform values: double roots come by themselves
b = src.build_bundle(0, 0, [r for r in roots])
lib = E.load_library()
image = lambda G, x: G.save_bundle(x).tobytes()
cut = lambda k, p: p * D // k


def build(G, cache_idx, part):
    part = np.ascontiguousarray(part)
    counts = np.full(bins, part.shape[1], dtype=np.uint32)
    h = C.c_void_p()
    E._check(lib.apsu_he_db_build_bundle(G.h, 0, cache_idx, C.c_void_p(part.ctypes.data), C.c_void_p(counts.ctypes.data), bins, part.shape[1], C.byref(h)))
    return E.Bundle(G, h, 0, cache_idx, part.shape[1])


def before(G, k):
    """bins -> host -> build_bundle per part in G"""
    counts = np.zeros(n, dtype=np.uint32)
    out = np.zeros((n, D), dtype=np.uint64)
    E._check(lib.apsu_he_bundle_bins(src.h, b.h, C.c_void_p(out.ctypes.data), C.c_void_p(counts.ctypes.data), C.c_uint32(D)))
    return [build(G, p, out[:bins, cut(k, p):cut(k, p + 1)]) for p in range(k)]


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


fmt = lambda v: "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))
rows = {"split": [], "spans": [], "adopt": [], "before-split": [], "before-adopt": []}
for rep in range(args.warmup + args.reps):
    w_split, parts = timed(lambda: src.split_bundle(b, 2))
    spans = src.split_times()
    w_adopt, moved = timed(lambda: dst.adopt_bundle(src, b))
    w_bs, old_parts = timed(lambda: before(src, 2))
    w_ba, old_moved = timed(lambda: before(dst, 1))
    if rep == 0:
        assert all(image(src, x) == image(src, y) for x, y in zip(parts, old_parts)), "a part differs from the build of the sliced roots"
        assert image(dst, moved) == image(dst, old_moved[0]), "the adopted BinBundle differs from the other context's build"
    if rep >= args.warmup:
        rows["split"].append(w_split); rows["spans"].append(spans); rows["adopt"].append(w_adopt)
        rows["before-split"].append(w_bs); rows["before-adopt"].append(w_ba)
    del parts, moved, old_parts, old_moved

names = ("decode + counts", "root search + multiplicities", "k_roots_split", "the two builds")
lines = [
    f"{args.params}: t = {t} ({t.bit_length()} bits), n = {n}, one BinBundle of {bins} bins x {D} items; ps_low_degree {src.info.ps_low_degree} -> "
    f"{dst.info.ps_low_degree} for the adopt; median (min .. max) of {args.reps} in ms, host wall time of the synchronous calls unless said otherwise",
    "  split into 2                          wall %s" % fmt(rows["split"]),
] + ["    device span: %-28s %s" % (nm, fmt([s[i] for s in rows["spans"]])) for i, nm in enumerate(names)] + [
    "  before: bins -> host -> 2 builds      wall %s" % fmt(rows["before-split"]),
    "  adopt into the other context          wall %s" % fmt(rows["adopt"]),
    "  before: bins -> host -> 1 build there wall %s" % fmt(rows["before-adopt"]),
    "  checked on the first repetition: both parts' images equal the builds of the sliced roots, the adopted image equals the other context's build",
]
text = "\n".join(lines) + "\n"
print(text, end="", flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
