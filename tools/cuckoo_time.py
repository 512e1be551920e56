"""N1, cuckoo hashing: apsu_he_item_locations at 1 M and 16 M items x 3 functions (device time of k_cuckoo_locations from the context's
events; wall time of the synchronous call with device pointers and with host pointers, copies included; the same cuckoo.h code on one
host core through libapsu_he_hostemu.so next to it), apsu_he_cuckoo_table's kernel in both table forms at 4096 items / 6552 slots and
11 041 / 16 380 with the rounds used, apsu_he_query_values at 16M-4096, and the compiler's resource report of the three kernels.
Median of --reps after --warmup.  Writes --out (and prints it)."""
import argparse, ctypes as C, os, re, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch, apsu_amd, emu_lib

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_cuckoo.txt"))
ap.add_argument("--hipcc", default="/opt/rocm/bin/hipcc")
args = ap.parse_args()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def params(name):
    return open(os.path.join(ROOT, "tests", "params", name + ".json")).read()


fmt = lambda v: "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


def measure(ctx, fn):
    """-> (wall ms list, device ms list of the call's kernels)"""
    wall, dev = [], []
    for rep in range(args.warmup + args.reps):
        ctx.profile_read(reset=True)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        if rep >= args.warmup:
            wall.append(dt * 1e3)
            dev.append(ctx.profile_read(reset=True)["other"][0])
    return wall, dev


rng = np.random.default_rng(24)
emu = emu_lib.load()
ctx = apsu_amd.HeContext(params("16M-4096"))
T, H = ctx.table_size, ctx.hash_func_count
say(f"median (min .. max) of {args.reps} in ms; {torch.cuda.get_device_name(0)}")
say(f"item_locations, 16M-4096: {H} functions, table_size {T}")
for count in (1 << 20, 1 << 24):
    items = rng.integers(0, 256, (count, 16), dtype=np.uint8)
    d_items = torch.from_numpy(items).cuda()
    d_locs = torch.empty(count * H, dtype=torch.int32, device="cuda")
    ctx.profile_enable(1)
    wall_d, dev = measure(ctx, lambda: ctx.item_locations(d_items.data_ptr(), count=count, locs=d_locs.data_ptr()))
    ctx.profile_enable(0)
    wall_dn, _ = measure(ctx, lambda: ctx.item_locations(d_items.data_ptr(), count=count, locs=d_locs.data_ptr()))
    wall_h, _ = measure(ctx, lambda: ctx.item_locations(items))
    out = np.zeros((count, H), dtype=np.uint32)
    t0 = time.perf_counter()
    emu.emu_cuckoo_locations(C.c_void_p(items.ctypes.data), C.c_uint64(count), C.c_uint32(H), C.c_uint32(T), C.c_void_p(out.ctypes.data))
    host_ms = (time.perf_counter() - t0) * 1e3
    assert (d_locs.cpu().numpy().view(np.uint32).reshape(count, H) == out).all()
    byts = count * (16 + 4 * H)
    kms = statistics.median(dev)
    say(f"  {count:9d} items: k_cuckoo_locations {fmt(dev)}   = {byts / kms / 1e6:.0f} GB/s of its {byts / 1e6:.0f} MB (16 B in, {4 * H} B out per item)")
    say(f"             wall, device pointers {fmt(wall_dn)}   wall, host pointers with copies {fmt(wall_h)}")
    say(f"             one host core, the same cuckoo.h code (tables included): {host_ms:.1f} ms")
    del d_items, d_locs

say("cuckoo_table: k_cuckoo_insert alone (locations given), by table form; wall = the debug call with host pointers and copies")
for name, count in (("16M-4096", 4096), ("16M-11041", 11041)):
    c2 = apsu_amd.HeContext(params(name))
    items = rng.integers(0, 256, (count, 16), dtype=np.uint8)
    locs = c2.item_locations(items)
    c2.profile_enable(1)
    for form, what in ((1, "LDS"), (2, "device memory")):
        try:
            _, _, rounds = c2.debug_cuckoo_insert(items, locs, c2.table_size, 500, form)
        except apsu_amd.ApsuHeError as e:
            say(f"  {count:6d} items / {c2.table_size:6d} slots, {what:13s}: refused ({str(e).split(': ', 1)[1]})")
            continue
        wall, dev = measure(c2, lambda: c2.debug_cuckoo_insert(items, locs, c2.table_size, 500, form))
        say(f"  {count:6d} items / {c2.table_size:6d} slots, {what:13s}: {rounds} rounds   kernel {fmt(dev)}   wall {fmt(wall)}")
    wall, dev = measure(c2, lambda: c2.cuckoo_table(items))
    say(f"  {count:6d} items / {c2.table_size:6d} slots, cuckoo_table (locations + table, the engine's form): kernels {fmt(dev)}   wall {fmt(wall)}")
    c2.close()

table_items = rng.integers(0, 256, (T, 16), dtype=np.uint8)
d_tab = torch.from_numpy(table_items).cuda()
d_vals = torch.empty(ctx.bundle_idx_count * ctx.n, dtype=torch.int64, device="cuda")
ctx.profile_enable(1)
wall, dev = measure(ctx, lambda: ctx.query_values(d_tab.data_ptr(), values=d_vals.data_ptr()))
wall_h, _ = measure(ctx, lambda: ctx.query_values(table_items))
say(f"query_values, 16M-4096 ({T} slots -> {ctx.bundle_idx_count} x {ctx.n} values): k_query_values {fmt(dev)}   wall, device pointers {fmt(wall)}   host pointers {fmt(wall_h)}")
ctx.close()

say("compiler's resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):")
with tempfile.TemporaryDirectory() as tmp:
    src = os.path.join(ROOT, "apsu_amd", "csrc", "kernels_cuckoo.hip")
    r = subprocess.run([args.hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                        os.path.join(tmp, "k.o"), src], capture_output=True, text=True)
    cur = None
    rows = {}
    for ln in r.stderr.splitlines():
        m = re.search(r"remark: +(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() or m.group(2)
            cur = re.sub(r"\(.*", "", cur).replace("void ", "").replace("apsu_he::", "")
            rows[cur] = {}
        elif cur:
            rows[cur][m.group(1).split(" ")[0]] = m.group(2)
    for k, v in rows.items():
        say(f"  {k:32s} VGPRs {v.get('VGPRs'):>3s}  AGPRs {v.get('AGPRs'):>2s}  SGPRs {v.get('TotalSGPRs'):>3s}  LDS {v.get('LDS'):>6s} B  scratch {v.get('ScratchSize')} B/lane  waves/SIMD {v.get('Occupancy')}")
        assert v.get("ScratchSize") == "0", "scratch must be 0"
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
