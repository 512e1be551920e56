"""CPU tier: tests/db_step_model.py, the integer model the GPU tier holds the resident-database kernels to, is itself held to the
oracle's polyn_with_roots and to the CPU emulation of the kernels (emu_bin_update, emu_bin_counts, emu_bins_lookup, emu_bins_merge,
emu_bins_eval, emu_bins_rows, emu_bin_roots) -- on every plain-modulus width of tests/test_gpu_db_kernel_steps.py and on its directed
inputs as far as the emulation's entries accept them (they take true counts and whole arrays, so poisoned rows above a top, caller-made
plans and the clamp stay with the GPU tier).  All comparisons are exact integers."""
import ctypes as C

import numpy as np
import pytest

import common
import db_step_model as M
from db_step_model import NONE, U, ints
import emu_lib
from emu_lib import vp
from oracle import ref

WIDTHS = [17, 28, 30, 31, 32, 33, 41, 50, 58]
RINGS = [64, 256]
u64p = C.POINTER(C.c_uint64)


def coeff_bits(bits):
    return (40, 40, 40, 36) if bits <= 33 else (60, 60, 60)


def db_json(n, bits):
    # felts_per_item so that an item's felts_per_item * (bits - 1) bits lie in the 80 .. 128 the parameters allow
    felts = 5 if bits <= 17 else 3 if bits <= 33 else 2
    return common.toy_json(n=n, coeff_bits=coeff_bits(bits), plain_bits=bits, ps_low=0, max_items=8300, felts=felts)


_REF = {}


def oracle(n, bits):
    if (n, bits) not in _REF:
        _REF[(n, bits)] = ref.RefContext.from_params(ref.load_params(db_json(n, bits)))
    return _REF[(n, bits)]


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


def directed_roots(rng, t, count):
    """root lists of one length: random, with 0 / 1 / t - 1, one value several times, all t - 1"""
    rnd = ints(rng.integers(0, t, count))
    out = [rnd, [t - 1] * count]
    if count >= 3:
        out.append([0, 1, t - 1] + rnd[3:])
        out.append([rnd[0]] * 3 + rnd[3:])
    return out


# ------------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("n", RINGS)
def test_every_width_is_a_context_and_the_product_of_linear_factors_is_the_oracles(n, bits):
    Cx = oracle(n, bits)
    t = int(Cx.t)
    assert t.bit_length() == bits and (t - 1) % (2 * n) == 0
    assert int(Cx.q[0]) > 2 * t                            # the stored plaintexts decode
    rng = np.random.default_rng([n, bits])
    for count in (0, 1, 2, 63, 64, 65, 200):
        for roots in directed_roots(rng, t, count):
            want = ints(Cx.polyn_with_roots(np.array(roots, dtype=np.uint64)))
            assert M.poly_from_roots(roots, t) == want


def test_the_engines_parameter_reader_accepts_every_context_of_the_gpu_tier(emu):
    for n, bits in [(n, b) for n in RINGS for b in WIDTHS] + [(4096, 17), (8192, 17)]:
        info = np.zeros(64, dtype=np.uint64)
        assert emu.emu_params_info(db_json(n, bits).encode(), info.ctypes.data_as(u64p), 64) > 0, (n, bits, emu.emu_last_error())


def test_kronecker_product_is_the_schoolbook_sum():
    rng = np.random.default_rng(1)
    for t in (int(oracle(64, 17).t), int(oracle(64, 58).t)):
        a, b = ints(rng.integers(0, t, 9)), ints(rng.integers(0, t, 5))
        want = [sum(a[i] * b[k - i] for i in range(9) if 0 <= k - i < 5) % t for k in range(13)]
        assert M.poly_mul(a, b, t) == want
        assert M.poly_mul([t - 1] * 70, [t - 1] * 70, t)[69] == 70 * (t - 1) ** 2 % t


# ------------------------------------------------------------------------------------------------------------ the update
def emu_update(emu, t, col, rem, ins):
    rows = len(col)
    a = np.array(col, dtype=np.uint64)
    out = np.full(rows, 0xDEAD, dtype=np.uint64)
    status = (C.c_int64 * 2)()
    r, i = np.array(list(rem) + [0], dtype=np.uint64), np.array(list(ins) + [0], dtype=np.uint64)
    cnt = emu.emu_bin_update(C.c_uint64(t), a.ctypes.data_as(u64p), C.c_uint32(rows), r.ctypes.data_as(u64p), C.c_uint32(len(rem)),
                             i.ctypes.data_as(u64p), C.c_uint32(len(ins)), out.ctypes.data_as(u64p), status)
    return cnt, ints(out), (status[0], status[1])


def model_update(t, col, rem, ins):
    poly = U(col).reshape(-1, 1)
    return M.bins_update(poly, [0], U(ins + [0]), [len(ins)], len(ins) + 1, U(rem + [0]), [len(rem)], len(rem) + 1, t)


def update_cases(rng, t):
    """(column, removals, insertions): Q (x - r) with every coefficient of Q at t - 1 and random Q, the top at 64 j - 1, 64 j, 64 j + 1;
    counts across a slot boundary both ways in one call; a double root out once and twice; failures at position 0 and later; zero"""
    out = []
    for top in (1, 63, 64, 65, 127, 128, 129):
        for Q in ([t - 1] * top, ints(rng.integers(0, t, top - 1)) + [int(rng.integers(1, t))]):
            for r in (0, 1, t - 1, int(rng.integers(0, t))):
                out.append((M.poly_mul(Q, [(-r) % t, 1], t), [r], []))
    roots = ints(rng.integers(0, t, 66))
    out.append((M.poly_from_roots(roots, t), roots[:4], []))                       # 66 -> 62
    out.append((M.poly_from_roots(roots[:62], t), [], roots[62:]))                 # 62 -> 66
    out.append((M.poly_from_roots(roots, t), roots[:4], ints(rng.integers(0, t, 70))))   # 66 -> 62 -> 132
    v = roots[5]
    twice = M.poly_from_roots(roots + [v], t)
    out += [(twice, [v], []), (twice, [v, v], []), (twice, [v, v, v], [])]          # the third time it is no root any more
    bad = next(x for x in range(2, t) if x not in roots)
    out += [(M.poly_from_roots(roots, t), [bad], [1]), (M.poly_from_roots(roots, t), roots[:3] + [bad] + roots[3:5], [1])]
    out.append(([0] * 70, [1], [2]))
    out.append(([t - 1], [1], []))                          # a constant has no root
    return out


@pytest.mark.parametrize("bits", WIDTHS)
def test_update_of_one_bin_is_the_emulations(emu, bits):
    t = int(oracle(64, bits).t)
    rng = np.random.default_rng([2, bits])
    for col, rem, ins in update_cases(rng, t):
        col = col + [0] * (len(ins) + 2)
        cnt, got, st = emu_update(emu, t, col, rem, ins)
        want, counts, st0, st1, failed = model_update(t, col, rem, ins)
        if st1 != M.NO_WORD:
            assert (cnt, st[0]) == (-1, 2)
        elif st0 != M.NO_WORD:
            assert (cnt, st[0], st[1]) == (-1, 1, st0 & 0xFFFFFFFF)
        else:
            assert st == (0, 0) and cnt == counts[0] and got == ints(want[:, 0])


# ------------------------------------------------------------------------------------------------------------ counts, lookup
def ragged_poly(rng, t, counts, rows, n, fill=None):
    """poly [rows][n]: column s arbitrary residues with its top non-zero coefficient at counts[s] (NONE: the zero column)"""
    poly = np.zeros((rows, n), dtype=np.uint64)
    for s, c in enumerate(counts):
        if c == NONE:
            continue
        poly[:c + 1, s] = rng.integers(0, t, c + 1, dtype=np.uint64) if fill is None else fill
        poly[c, s] = max(int(poly[c, s]), 1)
    return poly


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("n", RINGS)
def test_counts_lookup_eval_and_rows_are_the_emulations(emu, n, bits):
    t = int(oracle(n, bits).t)
    rng = np.random.default_rng([3, n, bits])
    for degree in list(range(10)) + [40]:
        rows = degree + 1
        counts = [int(c) for c in rng.integers(0, rows, n)]
        counts[0], counts[1], counts[n - 1] = degree, NONE, 0
        poly = ragged_poly(rng, t, counts, rows, n, fill=(t - 1) if degree % 2 else None)
        got = np.zeros(n, dtype=np.uint32)
        emu.emu_bin_counts(vp(poly), C.c_uint64(n), C.c_uint32(rows), vp(got))
        assert ints(got) == M.bin_counts(poly) == counts
        assert M.poly_degree(poly) == degree
        # the lookup: F = 3 points per entry from 0, 1, t - 1, true roots and random values; up to LOOKUP_R + 1 entries per start bin
        F, entries = 3, []
        for e in range(24):
            s = int(rng.integers(0, n - F + 1)) if e % 3 else (e // 3) % 2
            entries.append((s, [[0, 1, t - 1, int(rng.integers(0, t))][int(rng.integers(0, 4))] for _ in range(F)]))
        col = ints(poly[:, 5])
        if M.top_of(col) >= 1:                              # a point that is a root of slot 5 if it has one over F_t (small t only)
            entries.append((5, [next(iter(M.field_roots(col, t)), 0) if t < 1 << 20 else 0, 0, 1]))
        felts = U([v for _, f in entries for v in f])
        start = np.array([s for s, _ in entries], dtype=np.uint32)
        flags = np.full(len(entries) * F, 0xEE, dtype=np.uint8)
        assert emu.emu_bins_lookup(C.c_uint64(t), vp(poly), C.c_uint64(n), C.c_uint32(degree), vp(felts), vp(start), C.c_uint64(len(entries)),
                                   C.c_uint32(F), M.LOOKUP_R, vp(flags), None) == 0
        work, pts, idx = M.lookup_plan(felts, start, F, n)
        assert all(1 <= w[2] <= M.LOOKUP_R for w in work)
        assert ints(flags) == M.bins_lookup(poly, work, pts, idx, [0xEE] * (len(entries) * F), t)
        # the plaintext answer
        x = U([[0, 1, t - 1, int(rng.integers(0, t))][s % 4] for s in range(n)])
        mask = U([t - 1 if s % 3 == 0 else int(rng.integers(0, t)) for s in range(n)])
        out, is_bin = np.full(n, 0xEE, dtype=np.uint64), np.full(n, 0xEE, dtype=np.uint8)
        assert emu.emu_bins_eval(C.c_uint64(t), vp(poly), C.c_uint64(n), C.c_uint32(rows), vp(x), vp(mask), 0, vp(out), vp(is_bin), None) == 0
        want, want_bin = M.bins_eval(poly, counts, x, mask, t)
        assert ints(out) == want and ints(is_bin) == want_bin
        # ragged rows of the first `bins` slots (all of them bins)
        c2 = [0 if c == NONE else c for c in counts]
        poly2 = ragged_poly(rng, t, c2, rows, n)
        bins = n - 7
        off = np.zeros(bins + 1, dtype=np.uint64)
        buf = np.full(sum(c + 1 for c in c2[:bins]) + 5, 0xEEEE, dtype=np.uint64)
        c32 = np.array(c2, dtype=np.uint32)
        total = emu.emu_bins_rows(vp(poly2), C.c_uint64(n), C.c_uint32(rows), vp(c32), C.c_uint32(bins), vp(off), vp(buf))
        assert total >= 0, emu.emu_last_error()
        want_off, want_rows = M.bins_rows(poly2, c2, bins)
        assert total == want_off[-1] and ints(off) == want_off and ints(buf) == want_rows + [0xEEEE] * 5


# ------------------------------------------------------------------------------------------------------------ the merge
def emu_merge(emu, t, A, B):
    out = np.full((A.shape[0] + B.shape[0] - 1, A.shape[1]), 0xEEEE, dtype=np.uint64)
    assert emu.emu_bins_merge(C.c_uint64(t), vp(A), A.shape[0] - 1, vp(B), B.shape[0] - 1, C.c_uint64(A.shape[1]), M.MERGE_K, 0, vp(out), None) == 0
    return out


def merge_walks(bits):
    """operand tops (both sides) whose longest walk is F - 1, F, F + 1 and 2 F + 1 steps for the fold interval F of the width; for the
    capped interval one shape of about 1100"""
    F = M.merge_fold_interval(bits)
    return [1100] if F == M.FOLD_CAP else sorted({max(w - 1, 0) for w in (F - 1, F, F + 1, 2 * F + 1) if w >= 1})


@pytest.mark.parametrize("bits", WIDTHS)
def test_merge_with_every_operand_at_t_minus_one_is_the_emulations(emu, bits):
    t = int(oracle(64, bits).t)
    assert M.merge_fold_interval(bits) == emu.emu_merge_fold_interval(bits)
    limit = 1 << (64 if bits <= 32 else 128)
    for top in merge_walks(bits):
        if top == 1100 and bits not in (17, 33, 58):
            continue                                        # (the capped interval is one code path: its three widths are the GPU tier's)
        A = np.full((top + 1, 64), t - 1, dtype=np.uint64)
        A[:, 1], A[1:, 2], A[0, 2] = 0, 0, 1                # slot 1 is no bin on this side, slot 2 holds the polynomial 1
        B = np.full((top + 1, 64), t - 1, dtype=np.uint64)
        B[:, 1] = 0
        tops = [top]
        for X, Y in ((A, B), (B, A)):
            want = M.bins_merge(X, tops, Y, tops, 2 * top + 1, t)
            assert (emu_merge(emu, t, X, Y) == want).all()
        worst = M.merge_largest_sum([t - 1] * (top + 1), [t - 1] * (top + 1), t)
        assert worst < limit
        F = M.merge_fold_interval(bits)
        if F != M.FOLD_CAP and top + 1 >= F:                # a whole interval of the uncapped ones goes to within one product of the limit
            assert limit - worst <= t * t


@pytest.mark.parametrize("bits", [17, 33, 58])
def test_merge_of_ragged_tiles_is_the_emulations(emu, bits):
    n = 256
    t = int(oracle(n, bits).t)
    rng = np.random.default_rng([4, bits])
    ca = [NONE] * 64 + [0] * 64 + [int(c) for c in rng.integers(0, 4, 64)] + [int(c) for c in rng.integers(0, 30, 64)]
    cb = [NONE] * 64 + [int(c) for c in rng.integers(0, 20, 64)] + [0] * 64 + [int(c) for c in rng.integers(0, 13, 64)]
    ca[130], cb[200], ca[250] = 3, 12, 29
    A, B = ragged_poly(rng, t, ca, 30, n), ragged_poly(rng, t, cb, 20, n)
    tops = lambda c: [max([-1] + [v for v in c[i:i + 64] if v != NONE]) for i in range(0, n, 64)]
    assert (emu_merge(emu, t, A, B) == M.bins_merge(A, tops(ca), B, tops(cb), 49, t)).all()


# ------------------------------------------------------------------------------------------------------------ the roots
@pytest.mark.parametrize("n", RINGS)
def test_roots_with_multiplicities_are_the_emulations(emu, n):
    t = int(oracle(n, 17).t)
    rng = np.random.default_rng([5, n])
    distinct = [int(v) for v in rng.permutation(t - 2)[:70] + 1]
    cases = [distinct[:5], distinct[:3] + [distinct[0]], [distinct[1]] * 3 + distinct[4:6], [distinct[2]] * 7, [0] + distinct[:4],
             [0, 0] + distinct[:3], [t - 1, t - 1, 1], distinct[:n - 1]]
    if n > 64:
        cases.append(distinct[:66] + [distinct[65]])
    cols = [M.poly_from_roots(r, t, lead=int(rng.integers(1, t))) for r in cases]
    cols.append(M.poly_mul(M.poly_from_roots(distinct[:2], t), next(p for p in ([c, 0, 1] for c in range(2, t)) if not M.field_roots(p, t)), t))
    for blocks in (1, 3):
        for col in cols:
            values, mult = np.full(len(col), 0xEEEE, dtype=np.uint64), np.full(len(col), 0xEE, dtype=np.uint32)
            words = U(col)
            found = emu.emu_bin_roots(n.bit_length() - 1, C.c_uint64(t), vp(words), len(col), blocks, vp(values), vp(mult), len(col))
            want = M.field_roots(col, t)
            assert found == len(want) and found <= len(col) - 1
            got_mult = ints(mult[:found]) if found < len(col) - 1 else [1] * found
            assert dict(zip(ints(values[:found]), got_mult)) == want
            assert (values[found:] == 0xEEEE).all()
    assert sum(M.field_roots(cols[-1], t).values()) == 2 < len(cols[-1]) - 1
