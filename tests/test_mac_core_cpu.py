"""CPU tier of the multiply-accumulate family: the functions the gfx950 kernels run (apsu_amd/csrc/mac_core.h: k_mac, k_term_product,
k_pack_rows, k_unpack_rows, the packed-row extraction) stepped over every lane of a launch's grid by the CPU emulation library and held
to big-integer arithmetic, and the launch plan (apsu_amd/csrc/mac_plan.h) held to a restatement of its rules.  Every comparison is exact.

The chains are test_gpu_mac_edges.py's: every width of its WIDTHS, its chain_lengths() around either form's chunk (or one chain of
200 terms), operands from edge_values.  Here the constants of a level are arguments, so a test can also pass the WRONG chunk and see
the sums wrap; and both grid orders run (on the GPU the second needs more than 65 535 jobs)."""
import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest

import edge_values as ev
import emu_lib
from emu_lib import vp
from mac_step_model import exact_chain
from oracle import ref
from test_gpu_mac_edges import LONG_CHAIN, WIDTHS, chain_lengths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAC_G = 4
PACKED_WIDTHS = [48, 49, 50, 52, 56, 64]
PAD = 16                                                  # bytes the engine keeps readable behind a bit-packed buffer


class MacJob(C.Structure):                                # MacJob of mac_core.h, as the device reads it
    _fields_ = [("pt", C.c_void_p * MAC_G), ("out", C.c_void_p * MAC_G), ("pw", C.c_void_p), ("cnt", C.c_uint32), ("ng", C.c_uint32),
                ("pt_stride", C.c_uint32), ("pw_stride", C.c_uint32), ("pw_poly_stride", C.c_uint32), ("out_poly_stride", C.c_uint32),
                ("limb0", C.c_uint32), ("nl", C.c_uint32), ("packed", C.c_uint32), ("pad", C.c_uint32)]


class TermJob(C.Structure):
    _fields_ = [("pt", C.c_void_p), ("pw", C.c_void_p), ("out", C.c_void_p)]


@pytest.fixture(scope="module")
def emu():
    lib = emu_lib.load()
    assert lib.emu_mac_job_bytes() == C.sizeof(MacJob) == 112
    return lib


def u32(v):
    return np.array(v, dtype=np.uint32)


def u64(v):
    return np.array(v, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def width_primes(bits):
    """the two data primes test_gpu_mac_edges.py runs this width on"""
    return tuple(ref.RefContext(8192, [bits] * 3, 0, 17).q[:2])


class Level:
    """the k_mac constants of a level's limbs; every one can be overridden"""

    def __init__(self, emu, qs, n, packed, chunk=None, chunk_k=None):
        self.qs = [int(q) for q in qs]
        self.n = n
        self.shift = [ev.mac_shift(q) for q in self.qs]
        self.chunk = list(chunk) if chunk else [ev.mac_chunk(q) for q in self.qs]
        self.chunk_k = list(chunk_k) if chunk_k else [rules(emu, q)[2] for q in self.qs]
        self.bits = [emu.emu_packed_row_bits(C.c_uint64(q)) if packed else 64 for q in self.qs]
        self.row_off = [sum(n * b // 8 for b in self.bits[:j]) for j in range(len(self.qs))]
        self.slot_bytes = sum(n * b // 8 for b in self.bits)

    def args(self):
        self.keep = (u64(self.qs), u32(self.shift), u32(self.chunk), u32(self.chunk_k), u32(self.bits))
        return (len(self.qs),) + tuple(vp(a) for a in self.keep) + (C.c_uint64(self.n),)


def rules(emu, q):
    out = np.zeros(4, dtype=np.uint32)
    emu.emu_mac_rules(C.c_uint64(int(q)), vp(out))
    return [int(v) for v in out]


def pack(emu, lv, dense):
    """dense [slots][L][n] -> the bit-packed slots, PAD readable bytes behind them"""
    slots = dense.shape[0]
    buf = np.full(slots * lv.slot_bytes + PAD, 0xA5, dtype=np.uint8)
    assert emu.emu_pack_rows(len(lv.qs), vp(u32(lv.bits)), C.c_uint64(lv.n), vp(dense), vp(buf), C.c_uint64(lv.slot_bytes), C.c_uint64(slots), 0, None) == 0
    return buf


class Chains:
    """jobs over one level: per job its powers [cnt][2][L][n], per stream its coefficients [cnt][L][n] and its output [2][L][n]"""

    def __init__(self, emu, lv, packed):
        self.emu, self.lv, self.packed = emu, lv, packed
        self.jobs, self.keep, self.streams = [], [], []

    def add(self, powers, coeffs):
        lv, L, n = self.lv, len(self.lv.qs), self.lv.n
        cnt = powers.shape[0]
        j = MacJob()
        j.pw = powers.ctypes.data
        j.cnt, j.ng, j.limb0, j.nl, j.packed, j.pad = cnt, len(coeffs), 0, L, int(self.packed), 0
        j.pw_stride, j.pw_poly_stride, j.out_poly_stride = 2 * L * n, L * n, L * n
        j.pt_stride = lv.slot_bytes if self.packed else L * n
        outs = []
        for g in range(MAC_G):                           # mac_plan: the missing streams of a short job alias stream 0
            src = g if g < len(coeffs) else 0
            if g < len(coeffs):
                data = pack(self.emu, lv, coeffs[g]) if self.packed else coeffs[g]
                out = np.full((2, L, n), 0xDEAD, dtype=np.uint64)
                self.keep.append(data)
                outs.append((data, out))
                self.streams.append((powers, coeffs[g], out))
            j.pt[g] = outs[src][0].ctypes.data
            j.out[g] = outs[src][1].ctypes.data
        self.keep.append(powers)
        self.jobs.append(j)

    def run(self, kara, limb_slow):
        arr = (MacJob * len(self.jobs))(*self.jobs)
        for _, _, out in self.streams:
            out[:] = 0xDEAD
        rc = self.emu.emu_mac(*self.lv.args(), arr, len(self.jobs), int(kara), int(self.packed), int(limb_slow))
        assert rc == 0, self.emu.emu_last_error()

    def expected(self):
        if not hasattr(self, "_exp"):                    # computed once, shared by the runs of a case
            self._exp = [np.stack([exact_chain(q, co[:, l], pw[:, :, l]) for l, q in enumerate(self.lv.qs)], axis=1) for pw, co, _ in self.streams]
        return self._exp

    def wrong(self):
        return [i for i, ((_, _, out), exp) in enumerate(zip(self.streams, self.expected())) if not (out == exp).all()]


def worst_case_chains(emu, qs, n, packed, lengths, seed):
    """one job per chain length (a width with one long chain: three jobs of it); stream counts 1, 3, 4 and the fills of edge_values in
    turn, so that every width sees every stream count and every fill; every stream's data differs"""
    lengths = lengths if len(lengths) >= 3 else list(lengths) * 3
    seen = set()
    lv = Level(emu, qs, n, packed)
    ch = Chains(emu, lv, packed)
    rng = np.random.default_rng(seed)
    L = len(qs)
    for x, cnt in enumerate(lengths):
        pf = ("max_halves", "q-1", "alternating")[x % 3]
        base = np.stack([ev.fill_poly(pf, qs, n, rng) for _ in range(2)])                       # [2][L][n]
        powers = np.ascontiguousarray(np.stack([np.roll(base, t % 7, axis=2) for t in range(cnt)]))
        coeffs = []
        for g in range((1, 3, 4)[x % 3]):
            cf = ev.FILLS[(x + g) % 4]
            seen |= {("streams", (1, 3, 4)[x % 3]), ("powers", pf), ("coefficients", cf)}
            one = ev.fill_poly(cf, qs, n, rng)
            c = np.stack([np.roll(one, (t + 3 * g) % 5, axis=1) for t in range(cnt)])
            c[cnt // 2, :, (g * 37) % n] = [(q - 1 - g) for q in qs]                            # no two streams of a job hold the same data
            coeffs.append(np.ascontiguousarray(c))
        ch.add(powers, coeffs)
    assert L == len(lv.qs) and len(seen) == 3 + 3 + 4
    return ch


@pytest.mark.parametrize("bits,packed", [(b, p) for b in WIDTHS for p in (0, 1)])
def test_worst_case_chains_every_width(emu, bits, packed):
    """chains around each chunk (or one long chain), every operand an extreme, both forms, both grid orders, one and two blocks of lanes.
    (At 59 and 60 bits the three-product form has chunks of 3 terms: the engine never launches it there, mac_kara_usable, but the
    arithmetic is exact and is held to the same sums.)"""
    qs = width_primes(bits)
    lengths = chain_lengths(qs)
    assert lengths == [LONG_CHAIN] or max(lengths) <= 2 * 127 + 1
    for n in (512, 1024):                                 # one block of 256 lanes; two blocks (at 49 bits every even window shift occurs)
        ch = worst_case_chains(emu, qs, n, packed, lengths, seed=bits * 2 + packed)
        for kara in (0, 1):
            for limb_slow in ((0, 1) if n == 512 else (1,)):
                ch.run(kara, limb_slow)
                assert ch.wrong() == [], "bits %d n %d three-product %d packed %d limb_slow %d" % (bits, n, kara, packed, limb_slow)


def test_window_shifts_at_49_bits(emu):
    """the claim above: 256 lanes of a 49-bit row meet every even shift of the 16-byte window"""
    assert {(k // 2) * 2 * 49 % 32 for k in range(0, 512, 2)} == set(range(0, 32, 2))


@pytest.mark.parametrize("bits,kara,factor,wraps", [(60, 0, 2, True), (58, 1, 2, False), (58, 1, 3, True)])
def test_wrong_chunk_wraps(emu, bits, kara, factor, wraps):
    """teeth: the same inputs with the chunk passed `factor` times too long give a wrong sum -- 60 bits: chunk 7 passed as 14.
    58 bits, three-product form, chunk 15: at 30 the MIDDLE sum of the maximum-halves fill does pass 2^64, and the result is still
    right: the cross sum is recovered as Smid - S00 - S11 modulo 2^64, so only its own size counts, and that one (two products of
    2^58 per term) passes 2^64 from 33 terms.  The multiple at which the fill wraps is therefore 3 (chunk 45), and there the sum is
    wrong.  Both claims are checked here in integers before the emulation runs."""
    qs = width_primes(bits)
    q = qs[0]
    s = ev.mac_shift(q)
    right = ev.mac_chunk_kara(q) if kara else ev.mac_chunk(q)
    assert right == (15 if kara else 7)
    wrong = right * factor
    cnt = 2 * wrong + 1
    m = ev.max_halves(q)
    lo, hi = m & ((1 << s) - 1), m >> s
    held = wrong - 2                                       # terms in the sums when k_mac folds (in_chunk + 3 > chunk), at the least
    assert (held * 2 * lo * hi >= 1 << 64) == wraps and (right - 1) * 2 * lo * hi < 1 << 64      # the cross sum
    if kara:
        assert held * (lo + hi) ** 2 >= 1 << 64 > (right - 1) * (lo + hi) ** 2                  # the middle sum: wraps at either multiple
    n = 512
    powers = np.ascontiguousarray(np.broadcast_to(np.stack([ev.fill_poly("max_halves", qs, n) for _ in range(2)]), (cnt, 2, 2, n)))
    coeffs = [np.ascontiguousarray(np.broadcast_to(ev.fill_poly("max_halves", qs, n), (cnt, 2, n)))]
    for chunks, ok in ((None, True), ([wrong, wrong], not wraps)):
        lv = Level(emu, qs, n, 0, chunk=None if kara else chunks, chunk_k=chunks if kara else None)
        ch = Chains(emu, lv, 0)
        ch.add(powers, coeffs)
        ch.run(kara, 1)
        assert (ch.wrong() == []) == ok


# ---- packed rows
def row_primes(w):
    """two moduli whose packed row is w bits wide (64: a 60-bit prime, stored dense)"""
    return width_primes(60 if w == 64 else w)


@pytest.mark.parametrize("w", PACKED_WIDTHS)
def test_pack_unpack_is_the_identity(emu, w):
    qs, n, slots = row_primes(w), 512, 3
    lv = Level(emu, qs, n, 1)
    assert lv.bits == [w, w]
    rng = np.random.default_rng(w)
    dense = np.stack([ev.fill_poly(("sprinkled", "q-1", "max_halves")[i], qs, n, rng) for i in range(slots)])
    buf = pack(emu, lv, dense)
    assert (buf[-PAD:] == 0xA5).all()                     # nothing written behind the slots
    back = np.zeros_like(dense)
    assert emu.emu_pack_rows(2, vp(u32(lv.bits)), C.c_uint64(n), None, vp(buf), C.c_uint64(lv.slot_bytes), C.c_uint64(slots), 1, vp(back)) == 0
    assert (back == dense).all()


@pytest.mark.parametrize("w", PACKED_WIDTHS)
def test_packed_coeff_agrees_with_packed_pair(emu, w):
    """the single-coefficient read (k_unpack_rows, k_limb0_rows) and the pair window (k_mac, k_term_product) on every coefficient"""
    qs, n = row_primes(w)[:1], 1024
    lv = Level(emu, qs, n, 1)
    dense = ev.fill_poly("sprinkled", qs, n, np.random.default_rng(w))[None]
    buf = pack(emu, lv, dense)
    pair = np.zeros(2, dtype=np.uint64)
    for k in range(0, n, 2):
        emu.emu_packed_pair(vp(buf), C.c_uint64(k), w, vp(pair))
        got = [emu.emu_packed_coeff(vp(buf), C.c_uint64(k), w), emu.emu_packed_coeff(vp(buf), C.c_uint64(k + 1), w)]
        assert got == [int(pair[0]), int(pair[1])] == [int(dense[0, 0, k]), int(dense[0, 0, k + 1])]


@pytest.mark.parametrize("bits,packed", [(50, 1), (56, 1), (60, 1), (56, 0), (30, 0)])
def test_term_product_is_a_chain_of_one_term(emu, bits, packed):
    qs, n = width_primes(bits), 1024
    lv = Level(emu, qs, n, packed)
    rng = np.random.default_rng(bits)
    powers = np.stack([ev.fill_poly(("alternating", "max_halves")[p], qs, n, rng) for p in range(2)])[None]   # [1][2][L][n]
    coeff = ev.fill_poly("sprinkled", qs, n, rng)[None]                                                      # [1][L][n]
    ch = Chains(emu, lv, packed)
    ch.add(np.ascontiguousarray(powers), [np.ascontiguousarray(coeff)])
    ch.run(0, 1)
    assert ch.wrong() == []
    data, chain_out = ch.keep[0], ch.streams[0][2]
    for limb in range(2):
        out = np.zeros((2, n), dtype=np.uint64)
        tj = (TermJob * 1)(TermJob(data.ctypes.data, powers.ctypes.data, out.ctypes.data))
        assert emu.emu_term_product(*lv.args(), tj, C.c_uint64(1), limb, 2 * n, n, packed) == 0
        assert (out == chain_out[:, limb]).all()


# ---- the launch plan
STREAM_FIELDS = ("pt", "pw", "out", "cnt", "pt_stride", "pw_stride", "pw_poly_stride", "out_poly_stride", "limb0", "nl", "packed")


def plan(emu, streams, qs, n, switch, want_jobs=True):
    flat = u64([[s[f] for f in STREAM_FIELDS] for s in streams]).reshape(-1)
    jobs = (MacJob * max(1, len(streams)))() if want_jobs else None
    info = np.zeros(7, dtype=np.uint64)
    rc = emu.emu_mac_plan(vp(flat), C.c_uint64(len(streams)), vp(u64(qs)), len(qs), C.c_uint64(n), switch, jobs, C.c_uint64(len(streams)), vp(info))
    assert rc == 0, emu.emu_last_error()
    keys = ("jobs", "units", "mean_cnt", "kara", "packed", "gx", "limb_slow")
    return dict(zip(keys, (int(v) for v in info))), jobs


def group_streams(streams):
    """restatement of the grouping: stable order by (pw, limb0, nl, cnt); runs of up to four streams that agree in everything but pt and out"""
    order = sorted(range(len(streams)), key=lambda i: tuple(streams[i][f] for f in ("pw", "limb0", "nl", "cnt")))
    same = [f for f in STREAM_FIELDS if f not in ("pt", "out")]
    jobs = []
    for i in order:
        s = streams[i]
        if jobs and len(jobs[-1]["pt"]) < MAC_G and all(jobs[-1][f] == s[f] for f in same) and not jobs[-1]["closed"]:
            jobs[-1]["pt"].append(s["pt"]); jobs[-1]["out"].append(s["out"])
        else:
            if jobs:
                jobs[-1]["closed"] = True
            jobs.append(dict({f: s[f] for f in same}, pt=[s["pt"]], out=[s["out"]], closed=False))
    return jobs


def test_plan_groups_streams_like_the_restatement(emu):
    rng = np.random.default_rng(5)
    qs = list(width_primes(56)) + [width_primes(50)[0]]
    streams = []
    for i in range(300):
        limb0, nl = ((0, 3), (0, 2), (2, 1))[int(rng.integers(0, 3))]
        streams.append(dict(pt=0x100000 + 4096 * i, pw=0x9000000 + 65536 * int(rng.integers(0, 5)), out=0x5000000 + 4096 * i, cnt=int(rng.choice([1, 44, 45])),
                            pt_stride=int(rng.choice([24576, 21504])), pw_stride=49152, pw_poly_stride=int(rng.choice([24576, 32768])), out_poly_stride=24576,
                            limb0=limb0, nl=nl, packed=int(rng.integers(0, 2))))
    rng.shuffle(streams)
    info, jobs = plan(emu, streams, qs, 8192, -1)
    want = group_streams(streams)
    assert info["jobs"] == len(want) and len(want) < len(streams)
    assert {len(w["pt"]) for w in want} == {1, 2, 3, 4}
    for j, w in zip(jobs, want):
        ng = len(w["pt"])
        assert [j.pt[g] for g in range(MAC_G)] == w["pt"] + [w["pt"][0]] * (MAC_G - ng)
        assert [j.out[g] for g in range(MAC_G)] == w["out"] + [w["out"][0]] * (MAC_G - ng)
        assert (j.pw, j.cnt, j.ng, j.pt_stride, j.pw_stride, j.pw_poly_stride, j.out_poly_stride, j.limb0, j.nl, j.packed, j.pad) == \
               (w["pw"], w["cnt"], ng, w["pt_stride"], w["pw_stride"], w["pw_poly_stride"], w["out_poly_stride"], w["limb0"], w["nl"], w["packed"], 0)
    bits = [emu.emu_packed_row_bits(C.c_uint64(q)) for q in qs]
    assert info["units"] == sum(s["cnt"] * sum(bits[l] if s["packed"] else 64 for l in range(s["limb0"], s["limb0"] + s["nl"])) for s in streams)
    assert info["mean_cnt"] == sum(s["cnt"] * s["nl"] for s in streams) // sum(s["nl"] for s in streams)
    assert info["packed"] == want[0]["packed"]


def one_stream(i, cnt=10, nl=2):
    return dict(pt=0x100000, pw=0x9000000 + 64 * i, out=0x5000000, cnt=cnt, pt_stride=16384, pw_stride=32768, pw_poly_stride=16384, out_poly_stride=16384,
                limb0=0, nl=nl, packed=0)


@pytest.mark.parametrize("n", [8192, 512, 32768])
def test_plan_grid_flips_between_65535_and_65536_jobs(emu, n):
    qs = width_primes(56)
    for njobs, limb_slow in ((1, 1), (65535, 1), (65536, 0), (70000, 0)):
        info, _ = plan(emu, [one_stream(i) for i in range(njobs)], qs, n, -1, want_jobs=False)
        assert (info["jobs"], info["limb_slow"], info["gx"]) == (njobs, limb_slow, (n // 2 + 255) // 256)


def all_parameter_primes():
    out = set()
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "params", "*.json"))):
        out |= set(ref.RefContext.from_params(ref.load_params(path)).q)
    return sorted(out)


def test_three_product_rule_matches_edge_values(emu):
    """mac_kara_usable(q) == (mac_chunk_kara(q) != 0), and the chunks build_level stores, for every prime of the parameter files and of WIDTHS"""
    assert len(glob.glob(os.path.join(ROOT, "tests", "params", "*.json"))) == 36
    primes = all_parameter_primes() + [q for b in WIDTHS for q in ref.RefContext(8192, [b] * 3, 0, 17).q]
    assert len(primes) > 40
    for q in primes:
        shift, chunk, chunk_k, usable = rules(emu, q)
        assert (shift, chunk) == (ev.mac_shift(q), ev.mac_chunk(q))
        assert bool(usable) == (ev.mac_chunk_kara(q) != 0)
        assert (chunk_k if usable else 0) == ev.mac_chunk_kara(q)
    assert [rules(emu, width_primes(b)[0])[3] for b in (58, 59, 60)] == [1, 0, 0]


def test_three_product_decision_of_the_plan(emu):
    """by chain length it switches at a mean of 96 terms; forced on it still needs every prime of the level to admit it"""
    ok, narrow = width_primes(56), width_primes(60)
    for cnt, switch, qs, kara in ((95, -1, ok, 0), (96, -1, ok, 1), (300, -1, ok, 1), (300, 0, ok, 0), (2, 1, ok, 1), (300, -1, narrow, 0), (300, 1, narrow, 0),
                                  (300, 1, [ok[0], narrow[0]], 0), (300, 1, [narrow[0], ok[0]], 0)):
        info, _ = plan(emu, [one_stream(i, cnt) for i in range(3)], qs, 8192, switch)
        assert info["kara"] == kara, (cnt, switch, qs)
    # the mean is over (stream, limb) chains: 95 and 97 terms -> 96
    info, _ = plan(emu, [one_stream(0, 95), one_stream(1, 97)], ok, 8192, -1)
    assert (info["mean_cnt"], info["kara"]) == (96, 1)
    info, _ = plan(emu, [one_stream(0, 95), one_stream(1, 96)], ok, 8192, -1)
    assert (info["mean_cnt"], info["kara"]) == (95, 0)
