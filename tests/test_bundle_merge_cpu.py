"""CPU tier of the BinBundle merge: (i) k_bins_merge as the waves run it (apsu_amd/csrc/bin_merge.h: lane = slot, a block of K output rows
per wave, the K-row window of B sliding under the walk over A's rows, lazy sums folded once per fold interval) stepped lane by lane by
the CPU emulation library (emu_bins_merge) and held to the big-integer convolution mod t; (ii) the compaction rule
(apsu_amd/csrc/db_compact.h through emu_plan_compaction) held to a checker that restates the rule.  All comparisons are exact integers."""
import ctypes as C
import glob
import itertools
import os

import numpy as np
import pytest

import emu_lib
from emu_lib import vp
from oracle import ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
T17 = 0x1C001                                             # 114689, a 17-bit batching prime
T32 = 4294967291                                          # 2^32 - 5, the widest prime below 2^32
T33 = 4294967311                                          # 2^32 + 15, the first prime above 2^32: 33 bits
T60 = (1 << 60) - 93                                      # the widest prime below 2^60


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


def is_prime(p):
    if p < 2 or p % 2 == 0:
        return p == 2
    d, s = p - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if a % p == 0:
            continue
        x = pow(a, d, p)
        if x in (1, p - 1):
            continue
        for _ in range(s - 1):
            x = x * x % p
            if x == p - 1:
                break
        else:
            return False
    return True


def param_moduli():
    """the plain modulus of every file in tests/params"""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "params", "*.json"))):
        with open(path) as f:
            p = ref.load_params(f.read())
        key = (p["n"], p["plain_modulus"], p["plain_bits"])
        if key not in out:
            out[key] = int(ref.RefContext.from_params(p).t)
    return sorted(set(out.values()))


# ------------------------------------------------------------------------------------------------------------ the product
def convolve(a, b, t):
    """big-integer convolution mod t: both coefficient lists packed into one integer each (Kronecker substitution), ONE product"""
    if not a or not b:
        return []
    width = (2 * t.bit_length() + max(len(a), len(b)).bit_length() + 7) // 8 + 1          # bytes per coefficient: no sum carries over
    pa = int.from_bytes(b"".join(int(v).to_bytes(width, "little") for v in a), "little")
    pb = int.from_bytes(b"".join(int(v).to_bytes(width, "little") for v in b), "little")
    prod = (pa * pb).to_bytes(width * (len(a) + len(b)), "little")
    return [int.from_bytes(prod[i * width:(i + 1) * width], "little") % t for i in range(len(a) + len(b) - 1)]


def test_convolve_is_the_schoolbook_sum():
    rng = np.random.default_rng(1)
    for t in (T17, T60):
        a = [int(v) for v in rng.integers(0, t, 7)]
        b = [int(v) for v in rng.integers(0, t, 4)]
        want = [sum(a[i] * b[k - i] for i in range(len(a)) if 0 <= k - i < len(b)) % t for k in range(10)]
        assert convolve(a, b, t) == want


def run_merge(emu, t, A, B, K, fold=0):
    """A [dA + 1][n], B [dB + 1][n] uint64 -> (C [dA + dB + 1][n], stats) or the refusal's text"""
    A, B = np.ascontiguousarray(A, dtype=np.uint64), np.ascontiguousarray(B, dtype=np.uint64)
    n = A.shape[1]
    Cc = np.full((A.shape[0] + B.shape[0] - 1, n), 0xEEEE, dtype=np.uint64)       # every word is written
    stats = np.zeros(3, dtype=np.uint64)
    rc = emu.emu_bins_merge(C.c_uint64(t), vp(A), A.shape[0] - 1, vp(B), B.shape[0] - 1, C.c_uint64(n), K, fold, vp(Cc), vp(stats))
    if rc != 0:
        return emu.emu_last_error().decode(), None
    return Cc, [int(v) for v in stats]


def model_merge(t, A, B):
    out = np.zeros((A.shape[0] + B.shape[0] - 1, A.shape[1]), dtype=np.uint64)
    for s in range(A.shape[1]):
        col = convolve([int(v) for v in A[:, s]], [int(v) for v in B[:, s]], t)
        out[:len(col), s] = col
    return out


def ragged(rng, t, counts, rows=None):
    """counts: per slot a count, or None for the zero polynomial -> [rows][n], monic of degree count, random below"""
    rows = rows or max([c for c in counts if c is not None] + [0]) + 1
    A = np.zeros((rows, len(counts)), dtype=np.uint64)
    for s, c in enumerate(counts):
        if c is None:
            continue
        A[:c, s] = [int(rng.integers(0, t)) for _ in range(c)]
        A[c, s] = 1
    return A


def check(emu, t, A, B, K):
    got, stats = run_merge(emu, t, A, B, K)
    assert stats is not None, got
    assert (got == model_merge(t, A, B)).all()
    return stats


def test_device_constants(emu):
    assert emu.emu_merge_k() == 8
    for bits in range(1, 61):
        assert emu.emu_merge_fold_exact(bits) == 1
        f, w = emu.emu_merge_fold_interval(bits), (64 if bits <= 32 else 128) - 2 * bits
        assert f == min(1 << w, 1024)
        # the bound itself, in Python integers: f worst products and a folded residue fit the accumulator
        m = (1 << bits) - 1
        assert f * m * m + m < 1 << (64 if bits <= 32 else 128)


@pytest.mark.parametrize("t", [T17, T33])
@pytest.mark.parametrize("K", [1, 3, 8, 16])
def test_random_ragged_bins(emu, t, K):
    rng = np.random.default_rng(K)
    n = 150                                                # three tiles, the last one partial
    ca = [None if s % 37 == 5 else int(rng.integers(0, 30)) for s in range(n)]
    cb = [None if s % 37 == 5 else int(rng.integers(0, 21)) for s in range(n)]
    for s in range(64, 128):                               # a tile of short bins: its walk is shorter than the others'
        ca[s], cb[s] = s % 3, s % 2
    check(emu, t, ragged(rng, t, ca), ragged(rng, t, cb), K)


def test_shapes_of_the_table(emu):
    rng = np.random.default_rng(7)
    K, t, n = 8, T17, 128
    # tile 0 holds one bin at max - 1 - c against c and only empty bins besides; tile 1 is ragged
    ca, cb = [0] * n, [0] * n
    ca[5], cb[5] = 7, 3
    for s in range(64, n):
        ca[s], cb[s] = int(rng.integers(0, 6)), int(rng.integers(0, 5))
    st = check(emu, t, ragged(rng, t, ca), ragged(rng, t, cb), K)
    assert st[0] == 2 * 2                                   # two tiles, rows 7 + 4 + 1 = 12 -> two row blocks
    # dA = 0: every bin of A is empty (the polynomial 1): the product is B
    A, B = ragged(rng, t, [0] * n), ragged(rng, t, cb)
    got, _ = run_merge(emu, t, A, B, K)
    assert (got == B).all()
    got, _ = run_merge(emu, t, B, A, K)
    assert (got == B).all()
    # dA < K with a partial last row block, and dA + dB + 1 an exact multiple of K
    for da, db in ((3, 9), (5, 3), (3, 12), (7, 8), (8, 7), (15, 16)):
        assert ((da + db + 1) % K == 0) == ((da, db) in ((3, 12), (7, 8), (8, 7), (15, 16)))
        ca = [int(rng.integers(0, da + 1)) for _ in range(n)]
        cb = [int(rng.integers(0, db + 1)) for _ in range(n)]
        ca[9], cb[70] = da, db
        check(emu, t, ragged(rng, t, ca), ragged(rng, t, cb), K)
    # slots beyond the bins hold the zero polynomial in both inputs: they stay zero
    ca = [3 if s < 100 else None for s in range(n)]
    got, _ = run_merge(emu, t, ragged(rng, t, ca), ragged(rng, t, ca), K)
    assert not got[:, 100:].any() and (got[6, :100] == 1).all()
    # a double root, and root 0: (x - 5)(x) times (x - 5)
    A, B = np.zeros((3, 64), dtype=np.uint64), np.zeros((2, 64), dtype=np.uint64)
    A[0], B[0] = 1, 1
    A[:, 2], B[:, 2] = [0, t - 5, 1], [t - 5, 1]
    got, _ = run_merge(emu, t, A, B, K)
    assert [int(v) for v in got[:, 2]] == [0, 25, t - 10, 1]


def test_zero_polynomial_in_exactly_one_input_is_an_error(emu):
    rng = np.random.default_rng(8)
    ca = [2, None, 1, None]
    for cb, slot in (([2, None, 1, 0], 3), ([None, None, 1, None], 0)):
        msg, stats = run_merge(emu, T17, ragged(rng, T17, ca), ragged(rng, T17, cb, rows=3), 8)
        assert stats is None and "slot %d " % slot in msg
    got, _ = run_merge(emu, T17, ragged(rng, T17, ca), ragged(rng, T17, ca), 8)
    assert not got[:, 1].any() and not got[:, 3].any()


def worst_case(emu, t, steps, K, fold=0):
    """every coefficient t - 1; the longest walk of a wave is `steps` steps (A has that many rows, B enough for the window never to
    run out), next to a shorter bin in the same tile"""
    assert steps % K == 0 or K == 1
    A = np.zeros((steps, 2), dtype=np.uint64)
    B = np.zeros((steps + 2 * K, 2), dtype=np.uint64)
    A[:, 0], B[:, 0] = t - 1, t - 1
    A[:3, 1], B[:2, 1] = t - 1, t - 1
    got, stats = run_merge(emu, t, A, B, K, fold)
    assert stats[2] == (steps + K - 1) // K * K
    return (got == model_merge(t, A, B)).all(), stats


def fold_of(emu, t):
    return emu.emu_merge_fold_interval(t.bit_length())


@pytest.mark.parametrize("t", [T17, T32, T33, T60] + param_moduli())
def test_worst_case_operands_around_the_fold_interval(emu, t):
    assert is_prime(t)
    f = fold_of(emu, t)
    for steps in (f - 1, f, f + 1):                        # K = 1: the walk is exactly that long
        if steps:
            ok, stats = worst_case(emu, t, steps, 1)
            assert ok, (t, steps)
            assert (stats[1] > 0) == (steps > f)           # a fold inside the walk exactly when the chain is longer than the interval
    K = 8                                                  # the device's K: walks come in chunks of K steps
    for steps in sorted({max(f // K - 1, 1) * K, (f + K - 1) // K * K, (f // K + 1) * K}):
        ok, _ = worst_case(emu, t, steps, K)
        assert ok, (t, steps)


@pytest.mark.parametrize("t", [T32, T60, (1 << 31) - 1])
def test_the_worst_case_is_sharp(emu, t):
    """where the interval is 2^(W - 2 bits) and not the cap, a chain a little more than twice as long overflows the sum: the check above
    would see an interval that was too long"""
    f = fold_of(emu, t)
    assert f < 1024
    ok, _ = worst_case(emu, t, 4 * f + 8, 1, fold=2 * f + 2)
    assert not ok


# ---------------------------------------------------------------------------------------------------------- plan_compaction
def run_plan(emu, counts, max_items):
    counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(len(counts), len(counts[0]) if len(counts) else 3)
    nb, n = counts.shape
    group, degree = np.full(nb, 99, dtype=np.uint32), np.full(nb, 99, dtype=np.uint32)
    groups = emu.emu_plan_compaction(vp(counts), nb, C.c_uint64(n), max_items, vp(group), vp(degree))
    assert groups >= 0
    return [int(g) for g in group], [int(d) for d in degree[:groups]]


def plan_errors(counts, max_items, group, degree):
    """the rule, restated as a check of a finished plan; -> list of what is wrong with it"""
    bad = []
    state = []                                             # per group: the counts as the walk has left them
    for b, c in enumerate(counts):
        fits = [g for g, gc in enumerate(state)
                if all((x == NONE) == (y == NONE) for x, y in zip(gc, c)) and all(x + y < max_items for x, y in zip(gc, c) if x != NONE)]
        g = group[b]
        if g > len(state):
            bad.append("group ids are not numbered by first member")
            return bad
        if g == len(state):
            if fits:
                bad.append("BinBundle %d fits group %d and was left alone" % (b, fits[0]))
            state.append(list(c))
            continue
        if any((x == NONE) != (y == NONE) for x, y in zip(state[g], c)):
            bad.append("BinBundle %d does not share group %d's bin set" % (b, g))
            return bad
        if g not in fits:
            bad.append("a bin sum of group %d reaches max_items_per_bin" % g)
        elif g != fits[0]:
            bad.append("BinBundle %d joined group %d, not the first that fits (%d)" % (b, g, fits[0]))
        state[g] = [x if x == NONE else x + y for x, y in zip(state[g], c)]
    for g, gc in enumerate(state):
        if any(x != NONE and x >= max_items for x in gc) and len([1 for x in group if x == g]) > 1:
            bad.append("a bin sum of group %d reaches max_items_per_bin" % g)
        if degree[g] != max([x for x in gc if x != NONE] + [0]):
            bad.append("degree of group %d" % g)
    if len(degree) != len(state):
        bad.append("number of groups")
    return bad


ALPHABET = [(0, 0, NONE), (1, 2, NONE), (2, 1, NONE), (3, 0, NONE), (0, 3, NONE), (1, 1, NONE), (1, 1, 1), (2, 0, 0), (NONE, NONE, NONE),
            (4, 0, NONE)]
MAX_ITEMS = 4                                             # 1 + 2 = 3 < 4 fits, 2 + 2 and 1 + 3 = 4 do not: both sides of the strict bound


def test_plan_compaction_over_every_small_tuple(emu):
    seen_merge = seen_refuse = 0
    for k in range(1, 5):
        for counts in itertools.product(ALPHABET, repeat=k):
            group, degree = run_plan(emu, counts, MAX_ITEMS)
            assert plan_errors(counts, MAX_ITEMS, group, degree) == [], (counts, group, degree)
            assert run_plan(emu, counts, MAX_ITEMS) == (group, degree)          # a function of the input alone
            seen_merge += len(set(group)) < k
            seen_refuse += len(set(group)) == k and k > 1
    assert seen_merge and seen_refuse
    # the bound from both sides, spelled out
    assert run_plan(emu, [(1, 2, NONE), (2, 1, NONE)], MAX_ITEMS) == ([0, 0], [3])
    assert run_plan(emu, [(1, 2, NONE), (1, 2, NONE)], MAX_ITEMS) == ([0, 1], [2, 2])
    assert run_plan(emu, [(1, 1, NONE), (1, 1, 1)], MAX_ITEMS) == ([0, 1], [1, 1])
    # first fit: the third BinBundle skips the group that is full and joins the next
    assert run_plan(emu, [(3, 0, NONE), (0, 0, NONE), (1, 1, NONE), (1, 2, NONE)], MAX_ITEMS) == ([0, 0, 1, 1], [3, 3])
    assert run_plan(emu, [], MAX_ITEMS) == ([], [])


def test_the_checker_flags_wrong_plans():
    a, b = (1, 2, NONE), (2, 1, NONE)
    assert plan_errors([a, b], MAX_ITEMS, [0, 0], [3]) == []
    assert any("left alone" in e for e in plan_errors([a, b], MAX_ITEMS, [0, 1], [2, 2]))
    assert any("reaches max_items_per_bin" in e for e in plan_errors([a, a], MAX_ITEMS, [0, 0], [4]))
    assert any("bin set" in e for e in plan_errors([(1, 1, NONE), (1, 1, 1)], MAX_ITEMS, [0, 0], [2]))
    assert any("not the first" in e for e in plan_errors([a, (0, 0, NONE), (0, 0, NONE)], MAX_ITEMS, [0, 1, 1], [2, 0]))
    assert any("degree" in e for e in plan_errors([a, b], MAX_ITEMS, [0, 0], [2]))
    assert any("numbered" in e for e in plan_errors([a, a], MAX_ITEMS, [0, 2], [2, 2]))


def test_merge_counts_names_the_first_slot(emu):
    a = np.array([1, 2, NONE, 3, 3], dtype=np.uint32)
    b = np.array([2, 1, NONE, 1, 1], dtype=np.uint32)
    out = np.zeros(5, dtype=np.uint32)
    assert emu.emu_merge_counts(vp(a), vp(b), C.c_uint64(5), 5, vp(out)) == 0
    assert [int(v) for v in out] == [3, 3, NONE, 4, 4]
    assert emu.emu_merge_counts(vp(a), vp(b), C.c_uint64(5), 4, vp(out)) == -1
    assert emu.emu_last_error().decode().startswith("bin 3:")
    b[2] = 0
    assert emu.emu_merge_counts(vp(a), vp(b), C.c_uint64(5), 5, vp(out)) == -1
    assert "slot 2 " in emu.emu_last_error().decode()


# ---------------------------------------------------------------------------------------------------------- merge_steps
def run_steps(emu, counts, degrees, max_items):
    """counts [n_bundles][n], degrees [n_bundles] -> (rows, tops [steps][2][tiles], degree), or (return code, the refusal's text)"""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    nb, n = counts.shape
    tiles = (n + 63) // 64
    deg = np.ascontiguousarray(degrees, dtype=np.uint32)
    rows, tops, degree = np.full(nb - 1, 99, dtype=np.uint32), np.full(2 * (nb - 1) * tiles, 99, dtype=np.int32), C.c_uint32(99)
    rc = emu.emu_merge_steps(vp(counts), vp(deg), nb, C.c_uint64(n), max_items, vp(rows), vp(tops), C.byref(degree))
    if rc != 0:
        return rc, emu.emu_last_error().decode()
    return [int(r) for r in rows], tops.reshape(nb - 1, 2, tiles).tolist(), degree.value


def model_steps(counts, degrees, max_items):
    """the definition in numpy: step k multiplies the product of BinBundles 0 .. k (its counts: the sums so far) by BinBundle k + 1.  The
    step's refusals come first: slot by slot, a bin in one operand only or (max_items != 0) a sum that reaches max_items; then an
    operand's largest count above its BinBundle's degree.  tops: per operand and tile of 64 slots the largest count, -1 without a bin;
    rows = the two operands' largest counts + 1; degree = the largest count of the last sums."""
    counts = np.asarray(counts, dtype=np.int64)
    nb, n = counts.shape
    tiles = (n + 63) // 64

    def tile_tops(c):
        return [max([int(v) for v in c[64 * k:64 * (k + 1)] if v != NONE], default=-1) for k in range(tiles)]

    run, rows, tops = counts[0].copy(), [], []
    for k in range(nb - 1):
        cb = counts[k + 1]
        lone = (run == NONE) != (cb == NONE)
        full = (run != NONE) & (cb != NONE) & (run + cb >= max_items) if max_items else np.zeros(n, dtype=bool)
        if (lone | full).any():
            s = int(np.argmax(lone | full))
            return -1, ("slot %d " % s) if lone[s] else ("bin %d:" % s)
        ta, tb = tile_tops(run), tile_tops(cb)
        if max(tb + [0]) > degrees[k + 1] or (k == 0 and max(ta + [0]) > degrees[0]):
            return -3, "merge: a bin count exceeds its BinBundle's degree"
        tops.append([ta, tb])
        rows.append(max(ta + [0]) + max(tb + [0]) + 1)
        run = np.where(run == NONE, NONE, run + cb)
    return rows, tops, max(tile_tops(run) + [0])


def check_steps(emu, counts, degrees, max_items):
    got, want = run_steps(emu, counts, degrees, max_items), model_steps(counts, degrees, max_items)
    if isinstance(want[0], int):
        assert got[0] == want[0] and want[1] in got[1], (got, want)
    else:
        assert got == want
    return got


def degrees_of(counts):
    return [max([int(v) for v in c if v != NONE] + [0]) for c in counts]


@pytest.mark.parametrize("n", [64, 128])
@pytest.mark.parametrize("nb", [2, 3])
def test_merge_steps_random_counts(emu, n, nb):
    rng = np.random.default_rng(100 * n + nb)
    for trial in range(20):
        counts = rng.integers(0, 7, (nb, n)).astype(np.int64)
        counts[:, rng.integers(0, n, 5)] = NONE           # the same slots are no bins in every input
        if n == 128 and trial % 2:
            counts[:, 64:] = NONE                          # a tile without a bin next to one with bins
        rows, tops, degree = check_steps(emu, counts, degrees_of(counts), 0)
        assert len(rows) == nb - 1 and degree <= 6 * nb
        if n == 128 and trial % 2:
            assert all(t[1] == -1 and t[0] >= 0 for step in tops for t in step)


def test_merge_steps_rows_are_a_bound_over_tiles(emu):
    # the largest counts of A and B in different slots of one tile: rows exceeds degree + 1, and with a third BinBundle of empty bins
    # the first step is the tallest
    a, b, c = [0] * 64, [0] * 64, [0] * 64
    a[3], b[40] = 5, 5
    rows, tops, degree = check_steps(emu, [a, b], [5, 5], 0)
    assert (rows, tops, degree) == ([11], [[[5], [5]]], 5) and rows[0] > degree + 1
    rows, tops, degree = check_steps(emu, [a, b, c], [5, 5, 0], 0)
    assert (rows, degree) == ([11, 6], 5) and rows[0] > rows[1] and tops[1] == [[5], [0]]
    # two tiles: each tile has its own tops, rows takes the largest of each operand wherever it lies
    a, b = [1] * 128, [2] * 128
    a[70], b[5] = 9, 4
    rows, tops, degree = check_steps(emu, [a, b], [9, 4], 0)
    assert (rows, tops, degree) == ([14], [[[1, 9], [4, 2]]], 11)
    # a BinBundle whose degree is above every count (plaintexts above the longest bin) is no error
    assert check_steps(emu, [a, b], [12, 4], 0) == (rows, tops, degree)


def test_merge_steps_refusals_in_order(emu):
    a = [2, 1, NONE, 3] + [0] * 60
    b = [1, 1, NONE, 1] + [0] * 60
    # the sum 3 + 1 = 4: max_items = 4 refuses it (a bin holds max_items - 1 at the most), 5 accepts it, 0 is no bound
    assert check_steps(emu, [a, b], [3, 1], 4)[0] == -1 and "bin 3:" in run_steps(emu, [a, b], [3, 1], 4)[1]
    assert check_steps(emu, [a, b], [3, 1], 5) == ([5], [[[3], [1]]], 4)
    assert check_steps(emu, [a, b], [3, 1], 0) == ([5], [[[3], [1]]], 4)
    # a slot that is a bin in one input only; an earlier slot's bound comes first
    lone = list(b)
    lone[2] = 0
    assert check_steps(emu, [a, lone], [3, 1], 5)[0] == -1 and "slot 2 " in run_steps(emu, [a, lone], [3, 1], 5)[1]
    assert "bin 0:" in run_steps(emu, [a, lone], [3, 1], 3)[1]
    # a count above its BinBundle's degree, in either operand of the first step and in the new operand of a later one: the logic error,
    # behind that step's merge_counts refusals
    for degrees in ([2, 1], [3, 0]):
        rc, msg = check_steps(emu, [a, b], degrees, 0)
        assert rc == -3 and msg == "merge: a bin count exceeds its BinBundle's degree"
    assert check_steps(emu, [a, b, b], [3, 1, 0], 0)[0] == -3
    assert check_steps(emu, [a, lone], [2, 1], 5)[0] == -1
    # the refusal of a later step: the sums so far count, 3 + 1 + 1 = 5
    assert "bin 3:" in run_steps(emu, [a, b, b], [3, 1, 1], 5)[1]
    assert check_steps(emu, [a, b, b], [3, 1, 1], 6) == ([5, 6], [[[3], [1]], [[4], [1]]], 5)
