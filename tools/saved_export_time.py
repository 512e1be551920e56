"""N2 towards the reference: apsu_he_bundle_export_saved on one full-degree BinBundle of 16M-4096 (8190 bins x 1303 items), the time
split by the context's own stamps (apsu_he_debug_export_times) into decode + counts, the root search of bundle_bins, k_bins_rows
(device time by events), the copies to the host, the plaintexts' serialisation (compr none and zstd) and the buffer's assembly, next
to the wall time of the call, the time to write the file and its size.  In the same run and on the same array the alternative to
k_bins_rows is measured: the decoded array poly[degree + 1][n] on the host, cut into the ragged rows with numpy's transposed copy (every bin of this BinBundle has the full count, so the rows are the transposed
array; one thread, column stride 8 n bytes).  The first export is reloaded and its image compared.
Median (min .. max) of --reps after --warmup, ms.  --out appends the lines to a file as well."""
import argparse, ctypes as C, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--params", default="16M-4096")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_saved_export.txt"))
args = ap.parse_args()

import numpy as np, apsu_amd
from apsu_amd import engine as E, seal, wire

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


js = open(os.path.join(ROOT, "tests", "params", args.params + ".json")).read()
ctx, sc = apsu_amd.HeContext(js), seal.SealContext(js)
t, n = ctx.t, ctx.n
bins = ctx.info.items_per_bundle * ctx.felts_per_item
D = ctx.max_items_per_bin - 1
rng = np.random.default_rng(1)
roots = rng.integers(0, t, (bins, D), dtype=np.uint64)
b = ctx.build_bundle(0, 0, [r for r in roots])
image = ctx.save_bundle(b).tobytes()
fmt = lambda v: "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))
say(f"{args.params}: t = {t} ({t.bit_length()} bits), n = {n}, {bins} bins x {D} items, degree {b.degree}, resident image {len(image) / 2**20:.1f} MiB; "
    f"median (min .. max) of {args.reps} after {args.warmup} warm-up, ms")

keys = ("decode_counts", "bundle_bins", "bins_rows", "copies", "serialise", "assemble")
names = ("decode + counts", "bundle_bins (search + multiplicities)", "k_bins_rows", "copies to the host", "plaintext serialisation", "buffer assembly")
first = None
with tempfile.TemporaryDirectory() as tmp:
    for compr, label in ((seal.COMPR_NONE, "none"), (seal.COMPR_ZSTD, "zstd")):
        wall, parts, write, size = [], [], [], 0
        for rep in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            buf = seal.export_saved_bundle(ctx, sc, b, compr=compr)
            w = (time.perf_counter() - t0) * 1e3
            ms = seal.export_saved_times(ctx)
            path = os.path.join(tmp, "bundle.bin")
            t0 = time.perf_counter()
            with open(path, "wb") as f:
                f.write(buf)
                f.flush()
                os.fsync(f.fileno())
            wr = (time.perf_counter() - t0) * 1e3
            if rep == 0:
                back, used = seal.upload_saved_bundle(ctx, sc, buf, 0)
                assert used == len(buf) and ctx.save_bundle(back).tobytes() == image, "the reload differs from the BinBundle"
                del back
                if first is None:
                    first = buf
            if rep >= args.warmup:
                wall.append(w); parts.append(ms); write.append(wr); size = len(buf)
        say(f"  compr {label}: wall {fmt(wall)}   file {size} bytes ({size / 2**20:.1f} MiB), written in {fmt(write)}")
        for k, name in zip(keys, names):
            say(f"    {name:40s} {fmt([p[k] for p in parts])}")

# the alternative: poly[degree + 1][n] on the host (here rebuilt from the exported rows: the same array), rows cut out on the host
lib = E.load_library()
u64p = C.POINTER(C.c_uint64)
keep = wire._buf(first)
nr, nf = C.c_size_t(), C.c_size_t()
E._check(lib.apsu_he_wire_bin_bundle_rows(keep, C.c_size_t(len(first)), 1, None, C.c_size_t(0), None, C.c_size_t(0), C.byref(nr), C.byref(nf)))
flat, off = np.zeros(nf.value, dtype=np.uint64), np.zeros(nr.value + 1, dtype=np.uint64)
E._check(lib.apsu_he_wire_bin_bundle_rows(keep, C.c_size_t(len(first)), 1, flat.ctypes.data_as(u64p), C.c_size_t(flat.size), off.ctypes.data_as(u64p),
                                          C.c_size_t(off.size), C.byref(nr), C.byref(nf)))
del keep, first
assert nr.value == bins
counts = (np.diff(off) - 1).astype(np.uint32)
poly = np.zeros((b.degree + 1, n), dtype=np.uint64)
for s in range(bins):
    poly[:counts[s] + 1, s] = flat[int(off[s]):int(off[s + 1])]
npt = []
assert (counts == b.degree).all()
for rep in range(args.warmup + args.reps):
    t0 = time.perf_counter()
    tr = np.ascontiguousarray(poly[:, :bins].T)
    c = (time.perf_counter() - t0) * 1e3
    if rep == 0:
        assert (tr.reshape(-1) == flat).all()
    if rep >= args.warmup:
        npt.append(c)
say(f"  host transposition of the downloaded array ({poly.nbytes / 2**20:.1f} MiB, column stride {8 * n} bytes) into the rows, numpy's transposed copy, one thread: {fmt(npt)}")
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
