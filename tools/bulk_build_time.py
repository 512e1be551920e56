"""N1, a whole database from its entries: apsu_he_db_build_from_entries on one full-size bundle index of 16M-4096 (about 12 M synthetic
post-OPRF entries over its 1638 locations, 6 to 7 BinBundles of up to 1303 items per bin), and next to the incremental path on an
entry count that path finishes in reasonable time.
  full    --entries entries, Poisson counts per location, all in bundle index 0: host wall time of the synchronous call and the device
          spans of apsu_he_debug_build_from_entries_times (the entries' copy, k_entries_scatter summed over the BinBundles, the builds),
          for every grid of --grids (workgroups per location; 0 = the engine's choice).  The scatter's bytes: 16 in and 8 F out per
          entry; its rate next to a plain device-to-device copy that moves the same number of bytes (half read, half written), timed
          with events in the same run.
  parent  --small entries: build_database against algebraize_items + apply_entries from no BinBundle (the only path before), wall
          time of both; the images are compared byte for byte.
Median (min .. max) of --reps after --warmup, written to --out (default: the next free profiles/rNN_bulk_build.txt)."""
import argparse, glob, os, re, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--params", default="16M-4096")
ap.add_argument("--entries", type=int, default=12_000_000)
ap.add_argument("--small", type=int, default=100_000)
ap.add_argument("--grids", default="0,1,2,6")
ap.add_argument("--out", default=None)
args = ap.parse_args()

import numpy as np, torch, apsu_amd

if args.out is None:
    taken = [int(m.group(1)) for m in (re.match(r"r(\d+)_", os.path.basename(p)) for p in glob.glob(os.path.join(ROOT, "profiles", "r*_*"))) if m]
    args.out = os.path.join(ROOT, "profiles", "r%02d_bulk_build.txt" % (max(taken + [0]) + 1))

G = apsu_amd.HeContext(open(os.path.join(ROOT, "tests", "params", args.params + ".json")).read())
T, F, ipb = G.table_size, G.felts_per_item, int(G.info.items_per_bundle)
cap = G.max_items_per_bin - 1
rng = np.random.default_rng(1)
fmt = lambda v: "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))
image = lambda b: G.save_bundle(b).tobytes()


def synthetic(total):
    """Poisson counts over the locations of bundle index 0, random 16-byte entries whose first 4 bytes count up (distinct per location)"""
    counts = np.zeros(T, dtype=np.uint64)
    counts[:ipb] = rng.poisson(total / ipb, ipb)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    count = int(offsets[-1])
    entries = np.frombuffer(rng.bytes(count * 16), dtype=np.uint8).reshape(count, 16).copy()
    entries[:, :4] = np.arange(count, dtype=np.uint32).view(np.uint8).reshape(count, 4)
    return entries, offsets


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def device_copy_ms(nbytes, reps=10):
    """a device-to-device copy of nbytes / 2 bytes: nbytes moved"""
    a = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    b.copy_(a)
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); b.copy_(a); e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


lines = []
# ---- full size
entries, offsets = synthetic(args.entries)
count = int(offsets[-1])
plan = G.entries_plan(offsets)
moved = count * (16 + 8 * F)
lines.append(f"{args.params}: n = {G.n}, F = {F}, {ipb} locations per bundle index, cap = {cap}; {count} entries in bundle index 0 "
             f"(largest location {int(np.diff(offsets).max())}) -> {int(plan[0])} BinBundles; median (min .. max) of {args.reps} in ms")
for grid in [int(g) for g in args.grids.split(",")]:
    G.set_scatter_blocks(grid)
    wall, spans = [], []
    for rep in range(args.warmup + args.reps):
        w, bundles = timed(lambda: G.build_database(entries, offsets))
        if rep >= args.warmup:
            wall.append(w); spans.append(G.build_times())
        degrees = [b.degree for b in bundles]
        del bundles
    scatter = [s[1] for s in spans]
    lines += [
        "  workgroups per location %d%s" % (grid, " (the engine's choice)" if grid == 0 else ""),
        "    wall                           %s" % fmt(wall),
        "    device span: copy of entries   %s" % fmt([s[0] for s in spans]),
        "    device span: k_entries_scatter %s   (%d launches, %.1f MB moved: %.1f GB/s)" % (fmt(scatter), len(degrees), moved / 1e6, moved / statistics.median(scatter) / 1e6),
        "    device span: the builds        %s" % fmt([s[2] for s in spans]),
    ]
G.set_scatter_blocks(0)
cp = device_copy_ms(moved)
lines.append("  plain device copy moving the same %.1f MB: %s  (%.1f GB/s); BinBundle degrees %s" % (moved / 1e6, fmt(cp), moved / statistics.median(cp) / 1e6, degrees))
del entries

# ---- against the incremental path
entries, offsets = synthetic(args.small)
(lo, hi, start), = [x for x in G.bucket_entries(offsets) if x[1] > x[0]]


def incremental():
    felts = G.algebraize_items(entries)
    return G.apply_entries([], inserts=(felts[lo:hi], start), bundle_idx=0).appended


w_new, w_old = [], []
for rep in range(args.warmup + args.reps):
    a, new = timed(lambda: G.build_database(entries, offsets))
    b, old = timed(incremental)
    if rep == 0:
        assert [image(x) for x in new] == [image(x) for x in old], "build_database differs from apply_entries from empty"
    if rep >= args.warmup:
        w_new.append(a); w_old.append(b)
    n_new = len(new)
    del new, old
lines += [
    f"  {int(offsets[-1])} entries in bundle index 0 -> {n_new} BinBundle(s), wall:",
    "    build_database                                  %s" % fmt(w_new),
    "    algebraize_items + apply_entries from empty     %s" % fmt(w_old),
    "    checked on the first repetition: the images are equal byte for byte",
]
text = "\n".join(lines) + "\n"
print(text, end="", flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
