"""GPU tier: every kernel under the resident-database calls, one launch at a time, bit for bit against the integer model.

apsu_he_debug_run_step (the steps from polyn_with_roots on, apsu_amd/csrc/engine_db_steps.cpp) puts chosen words in front of ONE
launch_* call of apsu_amd/csrc/device.h with make_mod(t) and the context's n; tests/db_step_model.py states the same step on Python
integers (held to the oracle and the CPU emulation by tests/test_db_step_model_cpu.py).  The public calls reach these kernels only with
polynomials that are products of (x - root) on toy shapes; here the operands are arbitrary residues, every templated instance runs at
its first and last shape, and the lazy sums of the merge are driven to their fold interval with every operand at t - 1.

Contexts: n = 64 (one tile of 64 slots) and n = 256 (four), plain moduli of 17, 28, 30, 31, 32, 33, 41, 50 and 58 bits, max_items 8300,
ps_low 0; the root search also at n = 4096 and 8192 (its two other instances).  Arrays are rows x n words.  Nothing is skipped, no
tolerance anywhere."""
import numpy as np
import pytest

import apsu_amd
import db_step_model as M
from apsu_amd.engine import STEP_COMPOSED, STEP_PLAN
from db_step_model import NONE, NO_WORD, U, ints
from test_db_step_model_cpu import WIDTHS, db_json, merge_walks, ragged_poly

pytestmark = pytest.mark.gpu

POISON = 0xDEADBEEFDEADBEEF                               # no residue of any t below 2^60
P32, P8 = 0xDEADBEEF, 0xEE
RINGS = [64, 256]


class Ctx:
    def __init__(self, n, bits):
        self.n, self.bits = n, bits
        self.G = apsu_amd.HeContext(db_json(n, bits))      # a context the library refuses is a finding, not a skip
        self.t = self.G.t
        assert self.t.bit_length() == bits and self.G.n == n and self.G.q[0] > 2 * self.t

    def run(self, step, ins, outs, **kw):
        kw.setdefault("batch", 0)
        self.G.debug_run_step(step, 0, ins=[None if x is None else np.ascontiguousarray(x, dtype=np.uint64) for x in ins], outs=outs, **kw)

    def rng(self, *key):
        return np.random.default_rng([self.n, self.bits] + [int(k) for k in key])


_CTX = {}


@pytest.fixture(scope="module")
def ctx():
    def get(n, bits):
        if (n, bits) not in _CTX:
            _CTX[(n, bits)] = Ctx(n, bits)
        return _CTX[(n, bits)]
    yield get
    for X in _CTX.values():
        X.G.close()
    _CTX.clear()


def same(got, want, what):
    got = np.asarray(got)
    want = U(want).reshape(got.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), "%s: %d words differ, first at %s: got %#x, want %#x" % (what, len(bad), tuple(bad[0]), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


def instance_shapes():
    """(id, slots instance or None for the serial kernel, first / last, the largest index the shape holds): first = one coefficient
    more than the instance below holds, last = all the instance holds; the serial kernels at the first shape past 128 slots"""
    out, prev = [], 0
    for S in M.SLOTS:
        form = "recursion" if S <= 32 else "slot-loop"
        out.append(pytest.param(S, 64 * prev, id="S%d-%s-first" % (S, form)))
        out.append(pytest.param(S, 64 * S - 1, id="S%d-%s-last" % (S, form)))
        prev = S
    out.append(pytest.param(None, 64 * prev, id="serial-first"))
    return out


def width_for(k):
    """the widths take turns over the instance shapes, so that every one of them meets register slots of every size"""
    return WIDTHS[k % len(WIDTHS)]


def special_roots(rng, t, count, kind):
    r = ints(rng.integers(0, t, count))
    if kind == 1:
        return [t - 1] * count
    if kind == 2 and count >= 3:
        r[0], r[count // 2], r[-1] = 0, 1, t - 1
    if kind == 3 and count >= 4:
        r[1] = r[2] = r[-1] = r[0]
    return r


# ================================================================ k_polyn_with_roots<SLOTS>, k_polyn_with_roots_serial
@pytest.mark.parametrize("n", RINGS)
@pytest.mark.parametrize("S, max_deg", instance_shapes())
def test_polyn_with_roots_every_instance_at_its_first_and_last_shape(ctx, S, max_deg, n):
    assert M.slots_instance(max_deg // 64 + 1) == S
    X = ctx(n, width_for(max_deg // 64 + n))
    t, rng = X.t, X.rng(1, max_deg)
    # (the serial kernel is one thread per bin and quadratic in the count: 8192 roots take it ten seconds, so the array's last row is
    # reached on one ring and the other stops at 2048)
    most = 2048 if S is None and n > 64 else max_deg
    counts = [min(max(c, 0), most) for c in (0, 1, 63, 64, 65, max_deg - 1, max_deg) + ((max_deg, 2, 0, 66) if n > 64 else ())]
    assert len(counts) % 4                                  # 7 or 11 bins: the last workgroup is not full
    stride = max_deg + 3
    roots = np.full((len(counts), stride), POISON, dtype=np.uint64)            # the words behind a count are not read
    for s, c in enumerate(counts):
        roots[s, :c] = U(special_roots(rng, t, c, s % 4))
    out = np.full((max_deg + 1, n), POISON, dtype=np.uint64)
    X.run("polyn_with_roots", [roots, U(counts)], [out], polys=len(counts), terms=stride, e0=max_deg)
    same(out, M.polyn_with_roots(roots.reshape(-1), counts, stride, max_deg, n, t), "polyn_with_roots")


# ================================================================ k_bins_update<SLOTS>, k_bins_update_serial
def update_columns(rng, t, rows):
    """(column, removals, insertions) whose counts stay below rows: removals from Q (x - r) with Q at t - 1 and random, the top at the
    last slot boundary and on either side of it and at the instance's top; counts taken down and up across a slot boundary in one
    call; a double root out once and twice; insertions up to the last row; the counts 0, 1, 63, 64, 65"""
    top = rows - 1
    cols = []
    tops = {top, top - 1} | {d for j in (top // 64,) for d in (64 * j - 1, 64 * j, 64 * j + 1)} | {1, 63, 64, 65}
    for k, d in enumerate(sorted(d for d in tops if 1 <= d <= top)):
        Q = [t - 1] * d if k % 2 == 0 else ints(rng.integers(0, t, d - 1)) + [int(rng.integers(1, t))]
        r = [0, 1, t - 1, int(rng.integers(0, t))][k % 4]
        cols.append((M.poly_mul(Q, [(-r) % t, 1], t), [r], []))
    if top >= 70:
        b = 64 * ((top - 3) // 64)                        # a slot boundary: from b + 2 down to b - 2 and up to b + 3
        roots = special_roots(rng, t, b + 2, 2)
        cols.append((M.poly_from_roots(roots, t, lead=t - 1), roots[:4], ints(rng.integers(0, t, 5))))
    # insertions alone, up to the last row (the serial kernel, one thread per bin, takes its last hundred only)
    for c in sorted({0, min(1, top), min(63, max(top - 1, 0))} if top < 8192 else {top - 100}):
        if c < top:
            cols.append((M.poly_from_roots(special_roots(rng, t, c, 3), t), [], special_roots(rng, t, top - c, 1 + c % 2)))
    if top >= 6:
        v = int(rng.integers(0, t))
        twice = M.poly_from_roots(ints(rng.integers(0, t, min(top, 66) - 2)) + [v, v], t)
        cols += [(twice, [v], [1]), (twice, [v, v], [])]
    cols.append(([t - 1], [], []))                        # a constant, named and left alone
    if len(cols) % 4 == 0:                                # the last workgroup is never full
        cols.append(([1], [], [t - 1]))
    return cols


def run_update(X, rows, cols, slots_of=None, seed=0):
    """the columns at chosen slots in an unordered touched list, every other column poison -> (got poly, got tail, want tuple)"""
    n, t = X.n, X.t
    rng = X.rng(2, rows, seed)
    assert len(cols) <= n
    slots = slots_of or [int(s) for s in rng.permutation(n)[:len(cols)]]
    poly = np.full((rows, n), POISON, dtype=np.uint64)
    is_, rs = max(len(c[2]) for c in cols) + 1, max(len(c[1]) for c in cols) + 1
    ins, rem = np.full((n, is_), POISON, dtype=np.uint64), np.full((n, rs), POISON, dtype=np.uint64)
    ic, rc = np.full(n, P32, dtype=np.uint64), np.full(n, P32, dtype=np.uint64)           # the counts of bins not named are not read
    for s, (col, r, i) in zip(slots, cols):
        poly[:, s] = U(col + [0] * (rows - len(col)))
        rem[s, :len(r)], ins[s, :len(i)], rc[s], ic[s] = U(r), U(i), len(r), len(i)
    touched = U(slots)
    want = M.bins_update(poly, touched, ins.reshape(-1), ic, is_, rem.reshape(-1), rc, rs, t)
    got, tail = poly.copy(), np.full(len(slots) + 2, P32, dtype=np.uint64)
    X.run("bins_update", [touched, ins, ic, rem, rc], [got, tail], terms=rows, batch=n, polys=is_, e0=rs)
    return got, tail, want


@pytest.mark.parametrize("n", RINGS)
@pytest.mark.parametrize("S, top", instance_shapes())
def test_bins_update_every_instance_and_both_removal_forms(ctx, S, top, n):
    rows = top + 1
    assert M.slots_instance((rows + 63) // 64) == S
    X = ctx(n, width_for(rows // 64 + n + 4))
    cols = update_columns(X.rng(3, rows), X.t, rows)
    assert len(cols) % 4                                    # the last workgroup is not full
    got, tail, (want, counts, st0, st1, failed) = run_update(X, rows, cols)
    assert not failed and (st0, st1) == (NO_WORD, NO_WORD)
    same(got, want, "bins_update: poly")                    # (the columns not named are the poison they were)
    same(tail, counts + [st0, st1], "bins_update: counts_out, status")


@pytest.mark.parametrize("S, top", [pytest.param(4, 255, id="S4-recursion"), pytest.param(48, 2200, id="S48-slot-loop"), pytest.param(None, 8192, id="serial")])
def test_bins_update_failures_report_the_lowest_bin_and_position(ctx, S, top):
    X = ctx(64, 31 if S == 48 else 41)
    t, rows, rng = X.t, top + 1, X.rng(4, top)
    roots = sorted(set(ints(rng.integers(0, t, top - 1))))
    bad = next(x for x in range(2, t) if x not in roots)
    good = M.poly_from_roots(roots, t)
    cols = [(good, [bad], [1]),                             # a non-root at position 0 ...
            (good, roots[:3] + [bad] + roots[3:5], []),     # ... and later in the list
            (good, roots[:2], [7]),                         # a bin that succeeds next to them
            ([0] * 5, [1], [2]), ([0] * 5, [], [3]),        # two zero columns
            (good, roots[:1] + [bad], [])]
    slots = [40, 9, 3, 50, 22, 12]
    got, tail, (want, counts, st0, st1, failed) = run_update(X, rows, cols, slots_of=slots)
    assert (st0, st1) == (9 << 32 | 3, 22) and sorted(failed) == [9, 12, 22, 40, 50]
    assert ints(tail[-2:]) == [st0, st1]
    assert ints(tail[:-2]) == [P32 if c is None else c for c in counts]           # a wave that stops writes no count
    keep = [s for s in range(64) if S is not None or s not in (9, 12, 40)]          # (the serial kernel divides in place: device.h)
    same(got[:, keep], want[:, keep], "bins_update: poly")


# ================================================================ k_bins_merge<NARROW>
MERGE_CASES = [pytest.param(bits, top, id="%s-t%d-F%d-walk%d" % ("u64" if bits <= 32 else "u128", bits, M.merge_fold_interval(bits), top + 1))
               for bits in WIDTHS for top in merge_walks(bits) if top != 1100 or bits in (17, 33, 58)]


@pytest.mark.parametrize("bits, top", MERGE_CASES)
def test_bins_merge_every_operand_at_t_minus_one_up_to_the_fold_interval(ctx, bits, top):
    X = ctx(64, bits)
    t, n = X.t, 64
    F = M.merge_fold_interval(bits)
    limit = 1 << (64 if bits <= 32 else 128)
    worst = M.merge_largest_sum([t - 1] * (top + 1), [t - 1] * (top + 1), t)
    assert worst < limit
    if F != M.FOLD_CAP and top + 1 >= F:
        assert limit - worst <= t * t                       # the accumulator is within one product of its limit
    A = np.full((top + 3, n), t - 1, dtype=np.uint64)
    A[top + 1:] = POISON                                    # rows above the tile's top are not read
    A[:top + 1, 1], A[1:top + 1, 2], A[0, 2] = 0, 0, 1      # slot 1: the zero polynomial, slot 2: the polynomial 1
    B = np.full((top + 1, n), t - 1, dtype=np.uint64)
    rows = 2 * top + 1 + M.MERGE_K + 3                      # not a multiple of MERGE_K, and one row block beyond topA + topB
    rows += rows % M.MERGE_K == 0
    assert rows % M.MERGE_K and (rows - 1) // M.MERGE_K * M.MERGE_K > 2 * top
    tops = np.array([top], dtype=np.int64).view(np.uint64)
    for P, Q in ((A, B), (B, A)):
        out = np.full((rows, n), POISON, dtype=np.uint64)
        X.run("bins_merge", [P, tops, Q, tops], [out], terms=rows)
        want = M.bins_merge(P, [top], Q, [top], rows, t)
        assert not want[2 * top + 1:].any() and int(want[top, 0]) == (top + 1) * (t - 1) ** 2 % t
        same(out, want, "bins_merge")


@pytest.mark.parametrize("bits", WIDTHS)
def test_bins_merge_four_tiles_with_tops_of_their_own(ctx, bits):
    X = ctx(256, bits)
    t, n, rng = X.t, 256, X.rng(5)
    ta, tb = [-1, 0, 3, 37], [5, 0, -1, 29]
    A, B = rng.integers(0, t, (40, n), dtype=np.uint64), rng.integers(0, t, (30, n), dtype=np.uint64)
    A[:, 64:70] = t - 1
    B[:, 64:70] = t - 1
    for X_, tp in ((A, ta), (B, tb)):
        for tl, top in enumerate(tp):
            X_[top + 1:, 64 * tl:64 * tl + 64] = POISON
    A[0, 200:210], A[1:38, 200:210] = 1, 0                  # the polynomial 1 in a tile with a large top
    for rows in (67, 16, 1):                                # the whole product; cut off at a block boundary; one row
        out = np.full((rows, n), POISON, dtype=np.uint64)
        X.run("bins_merge", [A, np.array(ta, dtype=np.int64).view(np.uint64), B, np.array(tb, dtype=np.int64).view(np.uint64)], [out], terms=rows)
        same(out, M.bins_merge(A, ta, B, tb, rows, t), "bins_merge rows %d" % rows)


# ================================================================ k_bins_eval<NARROW>
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("n", RINGS)
def test_bins_eval_heads_tails_clamp_and_the_bad_flag(ctx, n, bits):
    X = ctx(n, bits)
    t, rng = X.t, X.rng(6)
    x = U([[0, 1, t - 1, int(rng.integers(0, t))][s % 4] for s in range(n)])
    mask = U([t - 1 if s % 3 == 0 else int(rng.integers(0, t)) for s in range(n)])

    def check(poly, counts, x, mask, what, bad=0, skip=()):
        out, tail = np.full(n, POISON, dtype=np.uint64), np.full(n + 1, P8, dtype=np.uint64)
        X.run("bins_eval", [poly, U(counts), x, mask], [out, tail], terms=poly.shape[0])
        want, is_bin = M.bins_eval(poly, counts, x, mask, t)
        keep = [s for s in range(n) if s not in skip]
        same(out[keep], [want[s] for s in keep], what)
        same(tail, is_bin + [bad], what + ": is_bin, bad")

    for top in list(range(18)) + [4000]:                    # around EVAL_ROWS = 8: the unrolled head against the tail
        rows = top + 1
        poly = rng.integers(0, t, (rows, n), dtype=np.uint64) if top % 2 else np.full((rows, n), t - 1, dtype=np.uint64)
        counts = [top] * n
        counts[1], counts[n - 1] = NONE, 0                  # not a bin: is_bin 0; the walk is the tile's all the same
        check(poly, counts, x, mask if top % 3 else None, "bins_eval top %d" % top)
    poly = rng.integers(0, t, (12, n), dtype=np.uint64)
    # a tile whose counts all say NONE reads nothing: out = mask; a top beyond the array is cut off at its last row
    counts = [NONE] * 64 + [11] * (n - 64) if n > 64 else [NONE] * n
    check(poly, counts, x, mask, "bins_eval: a tile without a bin")
    check(poly, [13 if s == 7 else 3 for s in range(n)], x, mask, "bins_eval: a count beyond the last row")      # 12 rows: the walk starts at row 11
    # a value that is not below t raises the flag; every other slot is what it was
    xb, mb = x.copy(), mask.copy()
    xb[3], mb[n - 2] = t, t
    check(poly, [11] * n, xb, mb, "bins_eval: x = t, mask = t", bad=1, skip=(3, n - 2))
    check(poly, [11] * n, xb, None, "bins_eval: x = t", bad=1, skip=(3,))
    check(poly, [11] * n, x, mask, "bins_eval afterwards")


# ================================================================ k_bins_lookup<LOOKUP_R>
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("n", RINGS)
def test_bins_lookup_head_tail_rows_per_work_item_and_poison(ctx, n, bits):
    X = ctx(n, bits)
    t, rng = X.t, X.rng(7)
    for degree in list(range(10)) + [4000]:                 # the 4-row head and its tail
        rows = degree + 1
        # columns with chosen roots: (x - a)(x - b) Q with a, b from 0, 1, t - 1 (Q arbitrary); slot 1 the zero column; the rest arbitrary
        poly = rng.integers(0, t, (rows, n), dtype=np.uint64)
        known = {}
        for s in range(2, 14):
            if degree >= 2:
                a, b = [0, 1, t - 1][s % 3], [1, t - 1, 0][s % 3]
                Q = ints(rng.integers(1, t, degree - 1)) if s % 2 else [t - 1] * (degree - 1)
                poly[:, s] = U(M.poly_mul(Q, M.poly_from_roots([a, b], t), t))
                known[s] = (a, b)
        poly[:, 1] = 0
        # slot s gets 1 .. 36 points (1 .. 9 under the long columns); the caller's plan cuts a tile's rows into work items of
        # 1, 2, .. LOOKUP_R rows, lookup_plan's own into LOOKUP_R and a rest
        most = 36 if degree < 100 else 9
        F, felts, start = 1, [], []
        for s in range(0, min(n, 80) if degree < 100 else 20):
            for k in range(1 + s % most):
                v = known[s][k % 2] if s in known and k < 2 else [0, 1, t - 1, int(rng.integers(0, t))][(s + k) % 4]
                felts.append(v)
                start.append(s)
        parts = len(felts)
        flags = np.full(parts + 3, P8, dtype=np.uint64)     # three parts nobody names
        whole, pts, idx = M.lookup_plan(felts, start, F, n, R=most)
        work = []
        for tile, row0, nrows in whole:
            r, k = 0, 0
            while r < nrows:
                take = min(1 + k % M.LOOKUP_R, nrows - r)
                work.append((tile, row0 + r, take))
                r, k = r + take, k + 1
        want = M.bins_lookup(poly, work, pts, idx, [P8] * (parts + 3), t)
        assert sum(want[:parts]) >= len(known) and not any(want[i] for i in range(parts) if start[i] == 1)       # 0 is "found" in no zero column
        assert degree >= 100 or {w[2] for w in work} == set(range(1, M.LOOKUP_R + 1))
        wk = U([[a, b, c, 0] for a, b, c in work])
        X.run("bins_lookup", [poly, wk, U(pts), U(idx)], [flags], terms=degree, flags=STEP_PLAN)
        same(flags, want, "bins_lookup degree %d (the caller's plan)" % degree)
        mine = np.full(parts, P8, dtype=np.uint64)           # lookup_plan's own plan names every part
        X.run("bins_lookup", [poly, U(felts), U(start)], [mine], terms=degree, polys=F)
        same(mine, want[:parts], "bins_lookup degree %d (lookup_plan)" % degree)


# ================================================================ k_bins_rows
@pytest.mark.parametrize("bits", [17, 33, 58])
@pytest.mark.parametrize("n", RINGS)
def test_bins_rows_writes_every_word_before_the_end_and_none_behind(ctx, n, bits):
    X = ctx(n, bits)
    t, rng = X.t, X.rng(8)
    rows = 130
    for bins in (n - 7, 1, 37):                             # below n and no multiple of 64
        counts = [[0, 63, 64, 65, 127, 128][int(k)] for k in rng.integers(0, 6, n)]
        counts[0] = 128
        for s in range(bins, n):
            counts[s] = NONE if s % 2 else 129              # behind the bins: not read
        poly = rng.integers(0, 1 << 63, (rows, n), dtype=np.uint64)               # any words: copied, no arithmetic
        want_off, want = M.bins_rows(poly, counts, bins)
        buf, off = np.full(len(want) + 9, POISON, dtype=np.uint64), np.zeros(bins + 1, dtype=np.uint64)
        X.run("bins_rows", [poly, U(counts)], [buf, off], terms=rows, polys=bins)
        same(off, want_off, "bins_rows: off")
        same(buf, want + [POISON] * 9, "bins_rows bins %d" % bins)


# ================================================================ k_bin_counts, k_poly_degree, k_eval_compare, k_unlift
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("n", RINGS)
def test_counts_degree_compare_and_unlift(ctx, n, bits):
    X = ctx(n, bits)
    t, q0, rng = X.t, X.G.q[0], X.rng(9)
    for rows in (1, 2, 9):
        for counts in ([NONE] * n, [0] * n, [rows - 1] * n, [NONE, 0, rows - 1, rows // 2] * (n // 4)):
            poly = ragged_poly(rng, 1 << 64, counts, rows, n)                      # any words
            got, deg = np.full(n, POISON, dtype=np.uint64), np.full(1, POISON, dtype=np.uint64)
            X.run("bin_counts", [poly], [got], terms=rows)
            X.run("poly_degree", [poly], [deg], terms=rows)
            assert ints(got) == M.bin_counts(poly) == counts and int(deg[0]) == M.poly_degree(poly)
    want = rng.integers(0, 1 << 64, (3, n), dtype=np.uint64)
    for where in ([], [(2, n - 1)], [(2, 5), (1, n - 1)], [(1, 7), (1, 6)], "all"):
        got = want.copy()
        if where == "all":
            got ^= np.uint64(1)
        for p, s in where if where != "all" else []:
            got[p, s] ^= np.uint64(1 << 63)
        status = np.full(2, POISON, dtype=np.uint64)
        X.run("eval_compare", [got, want], [status], polys=3)
        assert (int(status[0]), int(status[1])) == M.eval_compare(got, want), where
    half = (t + 1) // 2
    x = U([0, 1, half - 1, half, t - 1, q0 - t, q0 - t + half - 1, q0 - t + half, q0 - 1] + ints(rng.integers(0, t, 300)) + ints(rng.integers(q0 - t, q0, 300)))
    y = np.full(len(x), POISON, dtype=np.uint64)
    X.run("unlift", [x], [y])
    same(y, M.unlift(x, t, q0), "unlift")
    assert int(y[5]) == 0 and int(y[8]) == t - 1


# ================================================================ k_bin_roots / gather + transform + scan, k_roots_mult
def roots_columns(rng, t, n):
    """root lists for the occupied bins: simple roots; multiplicities 2, 3 and all; the root 0 once and twice; t - 1; more than 64
    distinct roots and one of them twice (the second pass of k_roots_mult's lanes) where the ring holds that many, n - 1 on the toy ring"""
    d = [int(v) for v in rng.permutation(t - 2)[:80] + 1]
    cases = [d[:5], d[:3] + [d[0]], [d[1]] * 3 + d[4:6], [d[2]] * 7, [0] + d[:4], [0, 0] + d[:3], [t - 1, t - 1, 1], d[:1], d[:2] + [d[1]] * 2]
    cases.append(d[:66] + [d[65]] if n > 64 else d[:n - 1])
    if n > 64:
        cases.append(d[:70] + [d[3]] * 2)
    return cases


ROOT_CASES = [pytest.param(64, 0, id="n64-persistent"), pytest.param(64, STEP_COMPOSED, id="n64-composed"), pytest.param(256, STEP_COMPOSED, id="n256-composed"),
              pytest.param(4096, 0, id="n4096-persistent"), pytest.param(4096, STEP_COMPOSED, id="n4096-composed"),
              pytest.param(8192, 0, id="n8192-persistent"), pytest.param(8192, STEP_COMPOSED, id="n8192-composed")]
_ROOTS = {}


def roots_input(X):
    """one array per ring, shared by both forms, with the model's answer"""
    if X.n not in _ROOTS:
        t, n, rng = X.t, X.n, np.random.default_rng([10, X.n])
        cases = roots_columns(rng, t, n)
        rows = max(len(c) for c in cases) + 1
        poly = np.zeros((rows, n), dtype=np.uint64)
        slots = sorted(int(s) for s in rng.permutation(n - 3)[:len(cases)] + 3)
        for s, c in zip(slots, cases):
            p = M.poly_from_roots(c, t, lead=int(rng.integers(1, t)))
            poly[:len(p), s] = U(p)
        # slot 0: a column that does not split (two roots and an irreducible quadratic); slot 1: a constant (a bin, but empty); slot 2: zero
        quad = next(p for p in ([c, 0, 1] for c in range(2, t)) if not M.field_roots(p, t))
        p = M.poly_mul(M.poly_from_roots(cases[0][:2], t), quad, t)
        poly[:len(p), 0], poly[0, 1] = U(p), 5
        _ROOTS[X.n] = (poly, M.roots_step(poly, t))
    return _ROOTS[X.n]


@pytest.mark.parametrize("n, form", ROOT_CASES)
def test_roots_both_forms_against_the_model(ctx, n, form):
    X = ctx(n, 17)
    poly, want = roots_input(X)
    assert [w[0] for w in want][:1] == [0] and sum(want[0][2].values()) == 2 < want[0][1]
    n_occ, hstride = len(want), max(w[1] for w in want) + 1
    # the toy ring's persistent form also with three workgroups: each takes many (bin, coset block) work items in turn
    for wgs in ((0, 3) if n == 64 and not form else (0,)):
        hits, tail = np.full(n_occ * hstride, POISON, dtype=np.uint64), np.full(n_occ + n_occ * hstride, P32, dtype=np.uint64)
        X.run("roots", [poly], [hits, tail], terms=poly.shape[0], e0=hstride, batch=wgs, flags=form)
        hits, found, mult = hits.reshape(n_occ, hstride), ints(tail[:n_occ]), tail[n_occ:].reshape(n_occ, hstride)
        for r, (s, cnt, mset) in enumerate(want):
            what = "bin %d (count %d)" % (s, cnt)
            assert found[r] == len(mset), what
            assert (hits[r, found[r]:] == POISON).all() and (mult[r, found[r]:] == P32).all(), what + ": a word behind `found` was written"
            got = ints(hits[r, :found[r]])
            assert sorted(got) == sorted(mset), what
            if found[r] < cnt:                              # fewer distinct roots than items: the multiplicities are written
                assert dict(zip(got, ints(mult[r, :found[r]]))) == mset, what
            else:
                assert (mult[r] == P32).all(), what


# ================================================================ refusals: nothing is launched, and the context goes on
def test_every_step_refuses_what_its_contract_does_not_admit(ctx):
    X = ctx(64, 33)
    t, n, q0 = X.t, 64, X.G.q[0]
    z = lambda *shape: np.zeros(shape, dtype=np.uint64)
    tops0 = z(1)
    bad = [
        ("polyn_with_roots", [U([[t, 0]]), U([1])], [z(3, n)], dict(polys=1, terms=2, e0=2)),                    # a root that is no residue
        ("polyn_with_roots", [U([[1, 0]]), U([3])], [z(3, n)], dict(polys=1, terms=2, e0=2)),                    # a count above its stride
        ("bins_update", [U([0]), z(n, 1), z(n), None, None], [z(0, n), z(3)], dict(terms=0, batch=n, polys=1)),  # rows of 0
        ("bins_update", [U([0]), z(n, 2), U([2] * n), None, None], [np.ones((2, n), dtype=np.uint64), z(3)], dict(terms=2, batch=n, polys=2)),   # count >= rows
        ("bins_update", [U([5, 5]), z(n, 1), z(n), None, None], [np.ones((2, n), dtype=np.uint64), z(4)], dict(terms=2, batch=n, polys=1)),      # a bin twice
        ("bins_update", [U([0]), z(n, 1), z(n), None, None], [np.full((2, n), t, dtype=np.uint64), z(3)], dict(terms=2, batch=n, polys=1)),      # no residue
        ("bin_counts", [z(0, n)], [z(n)], dict(terms=0)),
        ("poly_degree", [z(2, n)], [z(2)], dict(terms=2)),                                                       # a wrong size
        ("bins_lookup", [np.full((2, n), t, dtype=np.uint64), U([1]), U([0])], [z(1)], dict(terms=1, polys=1)),
        ("bins_lookup", [z(2, n), U([1]), U([n])], [z(1)], dict(terms=1, polys=1)),                              # a start bin beyond the slots
        ("bins_lookup", [z(2, n), U([[0, 0, M.LOOKUP_R + 1, 0]]), z(16, 64), np.full((16, 64), NONE, dtype=np.uint64)], [z(1)], dict(terms=1, flags=STEP_PLAN)),
        ("bins_lookup", [z(2, n), U([[0, 0, 1, 0]]), z(1, 64), np.full((1, 64), 1, dtype=np.uint64)], [z(1)], dict(terms=1, flags=STEP_PLAN)),   # a part beyond flags
        ("bins_merge", [z(2, n), U([2]), z(2, n), tops0], [z(3, n)], dict(terms=3)),                              # a top beyond the array
        ("bins_merge", [np.full((2, n), t, dtype=np.uint64), U([1]), z(2, n), tops0], [z(3, n)], dict(terms=3)),
        ("bins_merge", [z(2, n), tops0, z(2, n), tops0], [z(0, n)], dict(terms=0)),
        ("bins_rows", [z(2, n), U([2] * n)], [z(8), z(3)], dict(terms=2, polys=2)),                              # a count >= rows
        ("bins_rows", [z(2, n), U([NONE] * n)], [z(8), z(3)], dict(terms=2, polys=2)),
        ("bins_eval", [np.full((2, n), t, dtype=np.uint64), z(n), z(n), None], [z(n), z(n + 1)], dict(terms=2)),
        ("bins_eval", [z(0, n), z(n), z(n), None], [z(n), z(n + 1)], dict(terms=0)),
        ("eval_compare", [z(0, n), z(0, n)], [z(2)], dict(polys=0)),
        ("roots", [z(2, n)], [z(1), z(2)], dict(terms=2, e0=1)),                                                   # a 33-bit modulus has too many cosets
        ("unlift", [U([t])], [z(1)], {}),                                                                        # between the two ranges
        ("unlift", [U([q0])], [z(1)], {}),
    ]
    for step, ins, outs, kw in bad:
        with pytest.raises(ValueError, match="debug_run_step"):
            X.run(step, ins, outs, **kw)
        out = z(3, n)                                       # the context is usable and right: (x - 1)(x - 2) in bin 0
        X.run("polyn_with_roots", [U([[1, 2]]), U([2])], [out], polys=1, terms=2, e0=2)
        assert ints(out[:, 0]) == [2, t - 3, 1] and not out[:, 1:].any(), step
    Y = ctx(64, 17)
    with pytest.raises(ValueError, match="degree >= n"):     # 65 rows: a degree of 64 does not fit a transform of 64 points
        Y.run("roots", [np.ones((65, n), dtype=np.uint64)], [z(n * 64), z(n + n * 64)], terms=65, e0=64)
    with pytest.raises(ValueError, match="no occupied bin"):
        Y.run("roots", [np.ones((1, n), dtype=np.uint64)], [z(1), z(2)], terms=1, e0=1)
