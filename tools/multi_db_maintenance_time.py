"""A resident database maintained on the multi-device handle (apsu_he_multi_db_*), timed next to the single context on the same
inputs.  16M-4096, ONE bundle index, four BinBundles: a full-degree one (every bin at max_items_per_bin - 1), two half-full ones
((max_items_per_bin - 1) // 2 items per bin) and a sparse one (16 items per bin).  Per device list (--devices, e.g. 0 and 0,0,0; on
three slots the four BinBundles lie on slots 0, 1, 2, 0):
  * lookup of 4096 entries against the four BinBundles;
  * apply_entries of 64 insertions + 64 removals: every repetition removes 64 other items of the full-degree BinBundle and inserts 64
    new entries, which the sparse BinBundle takes -- two BinBundles are rebuilt per call;
  * compact: the two half-full BinBundles become one (they are removed and built again, untimed, between repetitions);
  * move_bundle of the full-degree BinBundle to the next slot (every repetition one slot further; one slot: nothing to move);
  * remove_bundle of the merged BinBundle (between the repetitions of compact): a commit on its own.
The single context runs lookup / apply_entries / compact on the same four BinBundles (it commits nothing, so every repetition sees the
same database).  Host wall time of the synchronous calls, median (min .. max) of --reps after --warmup, in ms."""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, apsu_amd

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--params", default="16M-4096")
ap.add_argument("--devices", action="append", help="a device list such as 0,0,0 (may be given several times; default: 0 and 0,0,0)")
args = ap.parse_args()
device_lists = [[int(v) for v in d.split(",")] for d in (args.devices or ["0", "0,0,0"])]

js = open(os.path.join(ROOT, "tests", "params", args.params + ".json")).read()
ctx = apsu_amd.HeContext(js)
t, F, n = ctx.t, ctx.felts_per_item, ctx.n
bins = ctx.info.items_per_bundle * F
D = ctx.max_items_per_bin - 1
H, SPARSE = D // 2, 16
rng = np.random.default_rng(1)
roots = {"full": rng.integers(0, t, (bins, D), dtype=np.uint64), "half_a": rng.integers(0, t, (bins, H), dtype=np.uint64),
         "half_b": rng.integers(0, t, (bins, H), dtype=np.uint64), "sparse": rng.integers(0, t, (bins, SPARSE), dtype=np.uint64)}
NAMES = ["full", "half_a", "half_b", "sparse"]           # cache_idx 0 .. 3
total = args.warmup + args.reps


def lookup_entries(count):
    """half of them items of the full-degree BinBundle (part j taken from bin s + j), half random values"""
    start = (rng.integers(0, bins // F, count) * F).astype(np.uint32)
    felts = rng.integers(0, t, (count, F), dtype=np.uint64)
    inside = np.arange(count) % 2 == 0
    col = rng.integers(0, D, count)
    for j in range(F):
        felts[inside, j] = roots["full"][start[inside] + j, col[inside]]
    return felts, start


def apply_batches():
    """per repetition 64 items of the full-degree BinBundle (column rep of 64 start bins: present, each once) and 64 new entries"""
    out = []
    for rep in range(total):
        start = (rng.choice(bins // F, 64, replace=False) * F).astype(np.uint32)
        rem = np.stack([roots["full"][start + j, rep] for j in range(F)], axis=1)
        ins_start = (rng.integers(0, bins // F, 64) * F).astype(np.uint32)
        out.append(((rng.integers(0, t, (64, F), dtype=np.uint64), ins_start), (np.ascontiguousarray(rem), start)))
    return out


def timed(fn, reset=None):
    times = []
    for rep in range(total):
        if reset:
            reset(rep)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn(rep)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        if rep >= args.warmup:
            times.append(dt * 1e3)
    return "%.3f (%.3f .. %.3f)" % (statistics.median(times), min(times), max(times))


entries = lookup_entries(4096)
batches = apply_batches()
print(f"{args.params}: {bins} bins, bundle index 0 holds four BinBundles of {D} / {H} / {H} / {SPARSE} items per bin; median (min .. max) of {args.reps} in ms")

single = [ctx.build_bundle(0, c, [r for r in roots[name]]) for c, name in enumerate(NAMES)]
want_present = ctx.lookup(single, entries)[0]
print("single context (HeContext, commits nothing)")
print("  lookup of 4096 entries, four BinBundles      : %s" % timed(lambda rep: ctx.lookup(single, entries)))
print("  apply_entries of 64 + 64                     : %s" % timed(lambda rep: ctx.apply_entries(single, inserts=batches[rep][0], removes=batches[rep][1])))
res = ctx.apply_entries(single, inserts=batches[0][0], removes=batches[0][1])
print("      states %s, %d removed, %d inserted, %d appended" % ([int(v) for v in res.state], int((res.rem_status == 2).sum()), int((res.ins_status == 0).sum()), len(res.appended)))
print("  compact (the two half-full ones merge)       : %s" % timed(lambda rep: ctx.compact(0, single)))
print("      groups %s" % [int(g) for g in ctx.compact(0, single).group])
del res

for devs in device_lists:
    M = apsu_amd.MultiContext(js, devs)
    world = len(devs)
    slot_of = lambda c: c % world
    for c, name in enumerate(NAMES):
        M.build_bundle(0, c, [r for r in roots[name]], slot=slot_of(c))
    print("handle over devices %s (slots of the four BinBundles: %s)" % (devs, [M.bundle_info(i).slot for i in range(4)]))
    assert (M.lookup(0, entries)[0] == want_present).all()
    print("  lookup of 4096 entries, four BinBundles      : %s" % timed(lambda rep: M.lookup(0, entries)))
    outcome = []
    print("  apply_entries of 64 + 64                     : %s" % timed(lambda rep: outcome.append(M.apply_entries(0, inserts=batches[rep][0], removes=batches[rep][1]))))
    r = outcome[-1]
    print("      last call: %d removed, %d inserted, %d appended, targets %s / %s" % (
        int((r.rem_status == 2).sum()), int((r.ins_status == 0).sum()), r.n_appended, sorted(set(int(v) for v in r.rem_target)), sorted(set(int(v) for v in r.ins_target))))

    def rebuild_halves(rep):
        if M.bundle_count() == 3:                            # the merged BinBundle has cache_idx 1: take it out, build the two again
            merged = next(i for i in range(3) if M.bundle_info(i).cache_idx == 1)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            M.remove_bundle(merged)
            remove_ms.append((time.perf_counter() - t0) * 1e3)
            for c in (1, 2):
                M.build_bundle(0, c, [r for r in roots[NAMES[c]]], slot=slot_of(c))
    made, remove_ms = [], []
    print("  compact (the two half-full ones merge)       : %s" % timed(lambda rep: made.append(M.compact(0)[1]), reset=rebuild_halves))
    assert set(made) == {1}, made
    rebuild_halves(0)
    # what a commit costs on its own: the wait for the owning engine, the renumbering and the release of one BinBundle's three arrays
    print("  remove_bundle of the merged BinBundle        : %.3f (%.3f .. %.3f)   [of %d]" % (statistics.median(remove_ms), min(remove_ms), max(remove_ms), len(remove_ms)))
    full_id = M.index_bundles(0)[0]
    if world > 1:
        b = ctx.save_bundle(single[0]).nbytes
        print("  move_bundle of the full-degree BinBundle     : %s   [%.1f MB device to device]" % (
            timed(lambda rep: M.move_bundle(full_id, (M.bundle_info(full_id).slot + 1) % world)), b / 1e6))
    else:
        print("  move_bundle of the full-degree BinBundle     : one slot, nothing to move")
    M.close()
