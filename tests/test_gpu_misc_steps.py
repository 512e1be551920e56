"""GPU tier: the ten launchers that no other family's steps reach -- launch_add, launch_clear_bits, launch_copy_jobs, launch_copy_sources,
launch_fill_random, launch_fill_blake2xb, launch_scatter_slots, launch_gather_slots, launch_algebraize, launch_pack_blocks -- one launch at
a time through the steps ADD .. PACK_BLOCKS of apsu_he_debug_run_step, against the models of tests/misc_step_model.py (held to the tree's
independent statements by tests/test_misc_step_model_cpu.py).  Contexts: n = 1024 with four 60-bit primes, n = 64 (below one workgroup),
n = 1024 with limbs of 36, 36 and 60 bits, and n = 4096 with five limbs, where a source ciphertext is longer than one grid stride of the
source check.  Every comparison is exact; guards hold what they held."""
import numpy as np
import pytest

import apsu_amd
import misc_step_model as M
import query_step_model
from misc_step_model import GUARD, M64, u64
from oracle import pymodel
from test_gpu_kernel_steps import chain_spec

pytestmark = pytest.mark.gpu

STRIDE = 64 * 256 * 2                                        # words one pass of the copy kernels' grid covers: 64 workgroups, 16 bytes a lane


class Ctx:
    def __init__(self, name, n):
        if name == "50x6-4096":
            q, t = pymodel.coeff_modulus_create(n, [50] * 6), pymodel.coeff_modulus_create(n, [17])[0]
        else:
            q, t, _ = chain_spec(name, n)
        self.n, self.t, self.first = n, t, len(q) - 2
        self.G = apsu_amd.HeContext(n=n, coeff_modulus=q, plain_modulus=t)
        self.q = [self.G.level_info(c)["q"] for c in range(self.first + 1)]
        self.clear_bits = self.G.level_info(0)["clear_bits"]
        assert all(self.q[c] == q[:c + 1] for c in range(self.first + 1))

    def run(self, step, c, ins, outs, **kw):
        self.G.debug_run_step(step, c, ins=ins, outs=outs, **kw)


_CTX = {}


@pytest.fixture(scope="module")
def ctx():
    def get(name, n=1024):
        if (name, n) not in _CTX:
            _CTX[(name, n)] = Ctx(name, n)
        return _CTX[(name, n)]
    yield get
    for X in _CTX.values():
        X.G.close()
    _CTX.clear()


SMALL = [("60x4", 1024), ("60x4", 64), ("36-36-60", 1024)]


# ------------------------------------------------------------------------------------------------------------- ADD, CLEAR_BITS
@pytest.mark.parametrize("name, n", SMALL)
def test_add(ctx, name, n):
    X = ctx(name, n)
    rng = np.random.default_rng(n)
    for c in range(X.first + 1):
        for polys, batch in ((1, 1), (2, 3), (3, 2), (3, 3)):
            a, b = M.add_operands(X.q[c], n, batch, polys, rng)
            acc = a.copy()
            X.run("add", c, [b], [acc], polys=polys, batch=batch)
            assert (acc == M.add(a, b, X.q[c], n)).all(), (name, c, polys, batch)
    a, b = M.add_operands(X.q[X.first], n, 1, 2, rng)
    for which in (0, 1):                                     # a word equal to its prime, in either operand: refused, nothing written
        ops = [a.copy(), b.copy()]
        ops[which][1, X.first, 5] = X.q[X.first][X.first]
        acc = ops[0].copy()
        with pytest.raises(ValueError, match="canonical"):
            X.run("add", X.first, [ops[1]], [acc], polys=2, batch=1)
        assert (acc == ops[0]).all()
    with pytest.raises(ValueError):
        X.run("add", X.first + 1, [b], [a.copy()], polys=2, batch=1)                 # no data level
    with pytest.raises(ValueError, match="wrong size"):
        X.run("add", X.first, [b], [a.copy()], polys=1, batch=1)


@pytest.mark.parametrize("name, n", SMALL[:2])
def test_clear_bits(ctx, name, n):
    X = ctx(name, n)
    rng = np.random.default_rng(7)
    for bits in sorted({0, 1, X.clear_bits, 63}):
        for words in (1, 255, 256, 257):
            w = rng.integers(0, 1 << 63, words + 1, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
            w[:min(words, len(M.CLEAR_WORDS))] = M.CLEAR_WORDS[:words]
            w[words - 1], w[words] = M64, M64                # all ones in the last word, and in the guard behind it
            out = w.copy()
            X.run("clear_bits", 0, [], [out], e0=bits)
            assert (out[:words] == M.clear_bits(w[:words], bits)).all() and out[words] == M64, (bits, words)
    for bits in (-1, 64):
        out = u64([5, 5])
        with pytest.raises(ValueError, match="bits"):
            X.run("clear_bits", 0, [], [out], e0=bits)
        assert out.tolist() == [5, 5]


# ------------------------------------------------------------------------------------------------------------- the copies
def test_copy_jobs(ctx):
    X = ctx("60x4", 1024)
    rng = np.random.default_rng(11)
    for words in (2, X.n, STRIDE, STRIDE + 2):               # the last: one grid stride and one pair
        for jobs in (1, 5) if words > 2 else (1, 2, 3, 4, 5):
            src = rng.integers(0, 1 << 63, (jobs, words), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
            out = np.full((jobs, words + 2), GUARD, dtype=np.uint64)
            X.run("copy_jobs", 0, [src], [out], terms=words, batch=jobs)
            assert (out[:, :words] == src).all() and (out[:, words:] == GUARD).all(), (words, jobs)
    for words in (0, 1, 3):
        with pytest.raises(ValueError):
            X.run("copy_jobs", 0, [np.zeros(max(words, 1), dtype=np.uint64)], [np.zeros(words + 2, dtype=np.uint64)], terms=words, batch=1)


def sources(X, c, jobs, rng):
    """clean sources [jobs][2][L][n]: random residues, q - 1 in the first and the last pair of every limb"""
    q, n = X.q[c], X.n
    s = np.zeros((jobs, 2, len(q), n), dtype=np.uint64)
    for j, m in enumerate(q):
        s[:, :, j] = rng.integers(0, m, (jobs, 2, n), dtype=np.uint64)
        s[:, :, j, [0, 1, n - 2, n - 1]] = m - 1
    return s


def run_sources(X, c, src, before, seq, in_place=False):
    out = src.copy() if in_place else np.full(src.shape, GUARD, dtype=np.uint64)
    rep = u64([GUARD])
    X.run("copy_sources", c, [None if in_place else src, u64([before, seq])], [out, rep], batch=len(src))
    assert (out == src).all()                                # copied whole, or left as it was
    return int(rep[0])


@pytest.mark.parametrize("name, n", SMALL + [("50x6-4096", 4096)])
def test_copy_sources_reports_a_bad_word_wherever_it_lies(ctx, name, n):
    X = ctx(name, n)
    rng = np.random.default_rng(n + len(name))
    seq = 1000
    for c in sorted({0, X.first}):                          # the one-limb form (words = 2 n) and the level's L
        q, L = X.q[c], c + 1
        words = 2 * L * n
        assert name != "50x6-4096" or c == 0 or words > STRIDE                  # the stride loop runs twice
        clean = sources(X, c, 1, rng)
        for in_place in (False, True):
            for before in (seq - 1, seq, seq + 1):
                assert run_sources(X, c, clean, before, seq, in_place) == before
        # per polynomial and limb: q_j - 1 passes (it is in `clean` at both ends), q_j is reported: in the first or the second word of a
        # pair; in the first pair, the last pair, and the first pair beyond the grid's stride
        spots = {0, 1, n - 2, n - 1}
        for p in range(2):
            for j in range(L):
                base = (p * L + j) * n
                for k in sorted(spots | {x - base for x in (STRIDE, STRIDE + 1) if base <= x < base + n}):
                    bad = clean.copy()
                    bad[0, p, j, k] = q[j]
                    for in_place in ((False, True) if k in (0, n - 1) else (False,)):
                        assert run_sources(X, c, bad, seq - 1, seq, in_place) == seq, (c, p, j, k, in_place)
        bad = clean.copy()
        bad[0, 1, L - 1, n // 2 + 1] = M64
        assert [run_sources(X, c, bad, b, seq) for b in (seq - 1, seq, seq + 1)] == [seq, seq, seq + 1]          # max(old, seq)
        assert [M.sources_report(bad, q, n, b, seq) for b in (seq - 1, seq, seq + 1)] == [seq, seq, seq + 1] and M.sources_report(clean, q, n, 3, seq) == 3
        # several jobs, one bad word in one of them
        many = sources(X, c, 3, rng)
        assert run_sources(X, c, many, 5, seq) == 5
        many[2, 0, 0, 7] = q[0]
        assert run_sources(X, c, many, 5, seq) == seq
    if name == "36-36-60":
        c = X.first
        q = X.q[c]
        assert q[0] < q[2] and q[1] < q[2]
        bad = sources(X, c, 1, rng)
        bad[0, 1, 0, 9] = q[0] + 5                           # at or above its own prime, far below the neighbouring limb's
        assert run_sources(X, c, bad, 0, seq) == seq
        bad[0, 1, 0, 9], bad[0, 1, 2, 9] = q[0] - 1, q[0] + 5                   # ... and the same word is fine in the wide limb
        assert run_sources(X, c, bad, 0, seq) == 0


# ------------------------------------------------------------------------------------------------------------- the generators
def test_fill_random(ctx):
    X = ctx("60x4", 1024)
    for seed in (0, M64, 0x243F6A8885A308D3):
        for bound in (1, 2, X.t, M64):
            for words in (1, 255, 256, 257):
                out = np.full(words + 1, GUARD, dtype=np.uint64)
                X.run("fill_random", 0, [u64([seed, bound])], [out])
                assert (out[:words] == M.fill_random(words, seed, bound)).all() and out[words] == GUARD, (seed, bound, words)
    out = u64([GUARD, GUARD])
    with pytest.raises(ValueError, match="bound of 0"):
        X.run("fill_random", 0, [u64([1, 0])], [out])
    assert (out == GUARD).all()


def test_fill_blake2xb(ctx):
    X = ctx("60x4", 1024)
    seed = np.random.default_rng(2).integers(0, 1 << 63, 8, dtype=np.uint64)
    for first in M.BLAKE_FIRST:
        for words in M.BLAKE_WORDS:
            for bound in ((1, X.t, (1 << 32) + 1) if words in (2, 17) else (X.t,)):
                out = np.full(words + 2, GUARD, dtype=np.uint64)
                X.run("fill_blake2xb", 0, [seed, u64([first, bound])], [out])
                assert (out[1:-1] == M.fill_blake2xb(words, seed, first, bound)).all(), (first, words, bound)
                assert out[0] == GUARD and out[-1] == GUARD, (first, words, bound)
    out = np.full(3, GUARD, dtype=np.uint64)
    with pytest.raises(ValueError, match="bound of 0"):
        X.run("fill_blake2xb", 0, [seed, u64([0, 0])], [out])
    with pytest.raises(ValueError, match="wrong size"):
        X.run("fill_blake2xb", 0, [seed[:7], u64([0, 5])], [out])
    assert (out == GUARD).all()


# ------------------------------------------------------------------------------------------------------------- the slots
@pytest.mark.parametrize("name, n", SMALL[:2])
def test_scatter_and_gather_slots(ctx, name, n):
    X = ctx(name, n)
    rng = np.random.default_rng(n)
    own = query_step_model.slot_map(n)
    for mp, given in ((own, None), (own, u64(own)), (M.rotation(n), u64(M.rotation(n)))):
        for batch in (1, 3):
            vals = rng.integers(0, 1 << 63, (batch, n), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
            s, g = np.full((batch, n), GUARD, dtype=np.uint64), np.full((batch, n), GUARD, dtype=np.uint64)
            X.run("scatter_slots", 0, [vals, given], [s], batch=batch)
            X.run("gather_slots", 0, [vals, given], [g], batch=batch)
            assert (s == M.scatter_slots(vals, mp)).all() and (g == M.gather_slots(vals, mp)).all()
            back = np.full((batch, n), GUARD, dtype=np.uint64)
            X.run("gather_slots", 0, [s, given], [back], batch=batch)
            assert (back == vals).all()                      # gather after scatter is the identity
    vals, out = np.zeros((1, n), dtype=np.uint64), np.full((1, n), GUARD, dtype=np.uint64)
    over, twice = u64(own), u64(own)
    over[3] = n
    twice[3] = twice[4]
    for step in ("scatter_slots", "gather_slots"):
        with pytest.raises(ValueError, match="at or above n"):
            X.run(step, 0, [vals, over], [out])
        with pytest.raises(ValueError, match="not a permutation"):
            X.run(step, 0, [vals, twice], [out])
    assert (out == GUARD).all()


# ------------------------------------------------------------------------------------------------------------- ALGEBRAIZE, PACK_BLOCKS
@pytest.mark.parametrize("felts, bpf, item_bits", M.ALGEBRAIZE_PARAMS)
def test_algebraize(ctx, felts, bpf, item_bits):
    X = ctx("60x4", 64)
    rng = np.random.default_rng(felts * bpf)
    counts = M.algebraize_counts(felts)
    # count * felts at 255, 256, 257 where felts divides one of them, else on either side of the workgroup's 256 lanes
    assert any(c * felts in (255, 256, 257) for c in counts) or min(counts) * felts < 256 < max(counts) * felts
    for count in counts + [140]:                             # 140: both constant items, the 128 walking ones, random ones
        items = M.algebraize_items(count, rng)
        out = np.full(count * felts + 1, GUARD, dtype=np.uint64)
        X.run("algebraize", 0, [items], [out], polys=felts, terms=bpf, e0=item_bits)
        assert (out[:-1] == M.algebraize(items, felts, bpf, item_bits)).all() and out[-1] == GUARD, count
    out = np.full(3, GUARD, dtype=np.uint64)
    for polys, terms, e0 in ((0, 20, 80), (2, 0, 80), (2, 65, 128), (3, 64, 128), (2, 20, 0), (2, 20, 129)):
        with pytest.raises(ValueError):
            X.run("algebraize", 0, [u64([[1, 2]])], [np.full(polys + 1, GUARD, dtype=np.uint64)], polys=polys, terms=terms, e0=e0)


@pytest.mark.parametrize("name, n", SMALL[:2])
def test_pack_blocks(ctx, name, n):
    X = ctx(name, n)
    rng = np.random.default_rng(n)
    for felts in M.PACK_FELTS:
        for ln in M.PACK_LENS:
            for batch, items in ((1, n // felts), (3, max(1, n // felts - 1)), (1, 1)):
                vals = rng.integers(0, 1 << 63, (batch, n), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (batch, n), dtype=np.uint64)
                vals[:, :2 * felts] = M64                    # every bit set: what the masks must cut
                out = np.full(batch * items * 2 + 1, GUARD, dtype=np.uint64)
                X.run("pack_blocks", 0, [vals], [out], polys=felts, terms=ln, e0=items, batch=batch)
                assert (out[:-1].reshape(batch, items, 2) == M.pack_blocks(vals, n, items, felts, ln)).all() and out[-1] == GUARD, (felts, ln, batch, items)
    vals = np.zeros((1, n), dtype=np.uint64)
    for polys, terms, e0 in ((0, 17, 1), (2, 1, 1), (2, 64, 1), (2, 17, 0), (2, 17, n // 2 + 1)):
        with pytest.raises(ValueError):
            X.run("pack_blocks", 0, [vals], [np.zeros(2 * max(e0, 1) + 1, dtype=np.uint64)], polys=polys, terms=terms, e0=e0)
