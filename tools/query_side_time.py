"""N5: time of the querier's side on the GPU -- query_create and relin_keygen -- beside the CPU oracle's encrypt / gen_relin_keys on
one core in the same run.  The oracle is this repository's C restatement of the reference's arithmetic, NOT Microsoft SEAL
(BASELINE.md).  Own process; warm-up, then `reps` repeats; median and spread (min .. max); device time from HIP events on the
context's stream, wall time from the host clock around the synchronous call.
    python tools/query_side_time.py [out.txt] [reps]
    python tools/query_side_time.py --once N    one warm query_create of N bundle indices at toy size and nothing else
                                                (for a kernel trace: the launch count must not depend on N)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch, apsu_amd
from oracle import ref

SEED = bytes(range(64))


def js_of(cfg):
    return open(os.path.join(ROOT, "tests", "params", cfg + ".json")).read()


def stats(v):
    v = sorted(v)
    return "%8.3f  (%.3f .. %.3f)" % (v[len(v) // 2], v[0], v[-1])


def timed(ctx, fn, reps, warm=3):
    """-> (device ms list, wall ms list) of the synchronous call fn()"""
    st = torch.cuda.ExternalStream(ctx.stream)
    dev, wall = [], []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        b.record(st)
        b.synchronize()
        if i >= warm:
            dev.append(a.elapsed_time(b)); wall.append((t1 - t0) * 1e3)
    return dev, wall


def cpu_timed(fn, reps):
    out = []
    for i in range(1 + reps):
        t0 = time.perf_counter(); fn(); t1 = time.perf_counter()
        if i:
            out.append((t1 - t0) * 1e3)
    return out


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--once":
        import common
        nb = int(sys.argv[2])
        ctx = apsu_amd.HeContext(common.toy_json(table_mult=4))
        sk = ctx.keygen(SEED)
        x = np.random.default_rng(1).integers(0, ctx.t, (nb, ctx.n), dtype=np.uint64)
        dev = torch.zeros(nb * ctx.source_power_count * 2 * (ctx.first_chain_idx + 1) * ctx.n, dtype=torch.int64, device="cuda")
        ctx.query_create(sk, list(range(nb)), x, dev.data_ptr(), seed=SEED)
        return
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    ref.set_threads(1)
    lines = ["querier side, %d repeats after warm-up: median (min .. max), milliseconds" % reps,
             "CPU columns: this repository's C restatement of the reference's arithmetic (oracle/), one core -- not SEAL", ""]
    for cfg, with_keys in (("16M-4096", True), ("256M-4096", False), ("1M-1024-com", False)):
        js = js_of(cfg)
        ctx = apsu_amd.HeContext(js)
        C = ref.RefContext.from_params(ref.load_params(js))
        n, S, L = ctx.n, ctx.source_power_count, ctx.first_chain_idx + 1
        idx = list(range(ctx.bundle_idx_count))
        count = len(idx) * S
        sk = ctx.keygen(SEED)
        x = np.random.default_rng(1).integers(0, ctx.t, (len(idx), n), dtype=np.uint64)
        xd = torch.from_numpy(x.view(np.int64)).cuda()
        dev = torch.zeros(count * 2 * L * n, dtype=torch.int64, device="cuda")
        d, w = timed(ctx, lambda: ctx.query_create(sk, idx, xd.data_ptr(), dev.data_ptr(), seed=SEED, values_on_device=True), reps)
        pts = [C.encode(x[c // S]) for c in range(count)]       # (the CPU column times the encryption alone, not the powers / encode)
        cpu = cpu_timed(lambda: [C.encrypt(sk, pts[c], 7 + c) for c in range(count)], max(3, reps // 4))
        lines += ["%s: n = %d, %d limbs, query_create of %d ciphertexts (%d bundle indices x %d source powers)" % (cfg, n, L, count, len(idx), S),
                  "  GPU device %s" % stats(d), "  GPU wall   %s" % stats(w), "  CPU encrypt x %d, one core %s" % (count, stats(cpu))]
        if with_keys:
            d, w = timed(ctx, lambda: ctx.relin_keygen(sk, SEED, want_host=False), reps)
            cpu = cpu_timed(lambda: C.gen_relin_keys(sk, 9), max(3, reps // 4))
            lines += ["%s: relin_keygen (%d keys x 2 x %d limbs), keys left resident on the device" % (cfg, ctx.K - 1, ctx.K),
                      "  GPU device %s" % stats(d), "  GPU wall   %s" % stats(w), "  CPU gen_relin_keys, one core %s" % stats(cpu)]
        lines.append("")
        ctx.close()
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
