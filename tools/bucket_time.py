"""N1, the database side's grouping by location: apsu_he_items_bucket (locations on the device, the counting sort and the caller's gather on
the host) next to apsu_he_items_bucket_device (the grouping and the gather on the device), on random items.
  rows    the parent's call (host wall time); the new call with order returned to the host (wall); the new call with order and entries
          left on the device (wall, and the device spans of apsu_he_debug_bucket_times: locations, grouping, gather).
  sizes   --items (default 16 M) and --small (1 M) items under --params (default 16M-4096: T = 6552, H = 3, two passes).
  rate    bytes a sort pass moves -- per key 8 read by the histogram, 8 read and 8 written by the scatter -- over a third of the grouping's
          span per pass (key generation and offsets/order take the rest: an upper bound on the passes' time, a lower bound on their rate),
          next to a plain device copy of the same bytes timed in the same run.
The first repetition checks offsets and order of the two calls against each other word for word, and entries against items[order].
Median (min .. max) of --reps after --warmup, written to --out (default: the next free profiles/rNN_bucket.txt)."""
import argparse, glob, os, re, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--params", default="16M-4096")
ap.add_argument("--items", type=int, default=16 * 1024 * 1024)
ap.add_argument("--small", type=int, default=1024 * 1024)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import numpy as np, torch, apsu_amd

if args.out is None:
    taken = [int(m.group(1)) for m in (re.match(r"r(\d+)_", os.path.basename(p)) for p in glob.glob(os.path.join(ROOT, "profiles", "r*_*"))) if m]
    args.out = os.path.join(ROOT, "profiles", "r%02d_bucket.txt" % (max(taken + [0]) + 1))

G = apsu_amd.HeContext(open(os.path.join(ROOT, "tests", "params", args.params + ".json")).read())
T, H = G.table_size, G.hash_func_count
bits = (T - 1).bit_length()
passes = -(-bits // 8)
fmt = lambda v: "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


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


def measure(count, reps, with_parent):
    items = np.frombuffer(np.random.default_rng(count).bytes(count * 16), dtype=np.uint8).reshape(count, 16)
    d_items = torch.from_numpy(items).cuda()
    d_order = torch.empty(count * H, dtype=torch.int32, device="cuda")
    d_entries = torch.empty(count * H * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    w_parent, w_gather, w_host, w_dev, spans = [], [], [], [], []
    total = 0
    for rep in range(args.warmup + reps):
        keep = rep >= args.warmup
        if with_parent or rep == 0:
            a, (off_p, order_p) = timed(lambda: G.bucket_items(items))
            if keep:
                w_parent.append(a)
            if rep == 0 or (keep and len(w_gather) < 3):                   # (three repetitions of the host gather: it is the longest row)
                g, ent_p = timed(lambda: items[order_p])
                if keep:
                    w_gather.append(g)
        b, (off_h, order_h, _, total) = timed(lambda: G.bucket_items_device(items, entries=False))
        c, (off_d, _, _, total_d) = timed(lambda: G.bucket_items_device(d_items.data_ptr(), count=count, order=d_order.data_ptr(), entries=d_entries.data_ptr()))
        if keep:
            w_host.append(b); w_dev.append(c); spans.append(G.bucket_times())
        if rep == 0:
            assert total == total_d == len(order_p) and (off_h == off_p).all() and (off_d == off_p).all() and (order_h == order_p).all()
            assert (d_order[:total].cpu().numpy().view(np.uint32) == order_p).all()
            assert (d_entries[:total * 16].cpu().numpy().reshape(total, 16) == ent_p).all()
            del ent_p
    sort = [s[1] for s in spans]
    moved = total * 24
    per_pass = statistics.median(sort) / passes
    cp = device_copy_ms(moved)
    lines = [f"  {count} random items -> {total} entries ({count * H - total} dropped: functions of an item on one location); checked on the first "
             "repetition: offsets, order and entries equal the parent's call and items[order], word for word"]
    if w_parent:
        lines += ["    apsu_he_items_bucket (parent: locations on the device, counting sort on the host), wall   %s" % fmt(w_parent),
                  "      the caller's gather items[order] on the host behind it, wall                             %s" % fmt(w_gather)]
    lines += [
        "    apsu_he_items_bucket_device, order to the host, wall                                      %s" % fmt(w_host),
        "    apsu_he_items_bucket_device, order and entries left on the device (items there too), wall %s" % fmt(w_dev),
        "      device span: k_cuckoo_locations  %s" % fmt([s[0] for s in spans]),
        "      device span: the grouping        %s   (3 launches for the keys, 3 per pass, 2 for offsets and order)" % fmt(sort),
        "      device span: k_entries_gather    %s   (%.1f MB moved: %.2f TB/s)" % (fmt([s[2] for s in spans]), total * 36 / 1e6, total * 36 / statistics.median([s[2] for s in spans]) / 1e9),
        "      a sort pass moves %.1f MB (8 B read by the histogram, 8 read and 8 written by the scatter, per key); at most 1/%d of the grouping's span each: "
        "%.3f ms, at least %.2f TB/s" % (moved / 1e6, passes, per_pass, moved / per_pass / 1e9),
        "      plain device copy moving the same %.1f MB: %s  (%.2f TB/s)" % (moved / 1e6, fmt(cp), moved / statistics.median(cp) / 1e9),
    ]
    return lines


lines = [f"{args.params}: table_size = {T}, hash_func_count = {H}: {bits} bits of location in {passes} passes; median (min .. max) in ms, "
         f"{args.reps} repetitions at {args.items} items, {max(3, args.reps // 4)} at {args.small}"]
lines += measure(args.items, args.reps, True)
lines += measure(args.small, max(3, args.reps // 4), True)
text = "\n".join(lines) + "\n"
print(text, end="", flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
