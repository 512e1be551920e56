"""CPU tier: the arithmetic of the BinBundle update (apsu_amd/csrc/bin_update.h) as k_bins_update runs it -- coefficient i in lane
i % 64, register slot i / 64, removal as a suffix scan over the 64 lanes with a carry between slots -- stepped lane by lane by the
CPU emulation library (emu_bin_update) and held to plain integer polynomial arithmetic mod t."""
import ctypes as C

import numpy as np
import pytest

import emu_lib

u64p = C.POINTER(C.c_uint64)
T = 0x1C001                                               # 114689 = 14 * 2^13 + 1, a 17-bit batching prime
COUNTS = [0, 1, 62, 63, 64, 65, 127, 128, 129, 200]


@pytest.fixture(scope="module")
def emu():
    lib = emu_lib.load()
    lib.emu_bin_unlift.argtypes = [C.c_uint64] * 3
    return lib


def poly_from_roots(roots, t=T, lead=1):
    p = [lead % t]
    for r in roots:
        q = [0] * (len(p) + 1)
        for i, c in enumerate(p):                         # p * (x - r)
            q[i + 1] = (q[i + 1] + c) % t
            q[i] = (q[i] - r * c) % t
        p = q
    return p


def divide(p, r, t=T):
    """p / (x - r) -> (quotient, remainder), plain synthetic division"""
    q, acc = [0] * (len(p) - 1), 0
    for k in range(len(p) - 1, 0, -1):
        acc = (p[k] + r * acc) % t
        q[k - 1] = acc
    return q, (p[0] + r * acc) % t


def run(emu, p, rem, ins, rows=None, t=T):
    rows = rows or max(len(p), len(p) - len(rem) + len(ins), 1) + 3
    a = np.zeros(rows, dtype=np.uint64)
    a[:len(p)] = p
    out = np.full(rows, 0xDEAD, dtype=np.uint64)
    status = (C.c_int64 * 2)()
    r = np.array(list(rem) + [0], dtype=np.uint64)
    i = np.array(list(ins) + [0], dtype=np.uint64)
    cnt = emu.emu_bin_update(C.c_uint64(t), a.ctypes.data_as(u64p), C.c_uint32(rows), r.ctypes.data_as(u64p), C.c_uint32(len(rem)),
                             i.ctypes.data_as(u64p), C.c_uint32(len(ins)), out.ctypes.data_as(u64p), status)
    return cnt, [int(v) for v in out], (status[0], status[1])


def expect(emu, p, rem, ins, want):
    cnt, out, st = run(emu, p, rem, ins)
    assert st == (0, 0) and cnt == len(want) - 1
    assert out[:len(want)] == want and not any(out[len(want):])


def roots_for(rng, count):
    return [int(v) for v in rng.integers(0, T, count)]


@pytest.mark.parametrize("before", COUNTS)
def test_every_count_before_and_after(emu, before):
    """insert-only, remove-only and mixed updates between all the counts that cross lane 63 -> 0 and the slot carry"""
    rng = np.random.default_rng(100 + before)
    roots = roots_for(rng, before)
    p = poly_from_roots(roots)
    for after in COUNTS:
        if after >= before:                               # insert-only
            ins = roots_for(rng, after - before)
            expect(emu, p, [], ins, poly_from_roots(roots + ins))
        if after <= before:                               # remove-only, in an order of its own
            gone = [roots[int(i)] for i in rng.permutation(before)[:before - after]]
            left = list(roots)
            for v in gone:
                left.remove(v)
            expect(emu, p, gone, [], poly_from_roots(left))
        # mixed: down to min(before, after) // 2 and up again
        keep = min(before, after) // 2
        gone, left = roots[keep:], roots[:keep]
        ins = roots_for(rng, after - keep)
        expect(emu, p, gone, ins, poly_from_roots(left + ins))


def test_root_zero_and_root_t_minus_one(emu):
    rng = np.random.default_rng(1)
    for c in (1, 64, 65, 130):
        roots = roots_for(rng, c - 1)
        for special in (0, T - 1):
            p = poly_from_roots(roots)
            expect(emu, p, [], [special], poly_from_roots(roots + [special]))
            expect(emu, poly_from_roots(roots + [special]), [special], [], p)
            expect(emu, poly_from_roots([special] + roots), [special], [special], poly_from_roots(roots + [special]))


def test_repeated_root_in_twice_out_once(emu):
    rng = np.random.default_rng(2)
    roots = roots_for(rng, 70)
    v = 4242
    twice = poly_from_roots(roots + [v, v])
    expect(emu, poly_from_roots(roots), [], [v, v], twice)
    expect(emu, twice, [v], [], poly_from_roots(roots + [v]))
    cnt, out, st = run(emu, poly_from_roots(roots + [v]), [v, v], [])      # ... and not a third time
    assert cnt == -1 and st == (1, 1)


def test_removing_a_non_root_reports_it_and_writes_nothing(emu):
    rng = np.random.default_rng(3)
    for c in (0, 1, 63, 64, 65, 129):
        roots = [int(v) for v in rng.choice(T - 1, size=c, replace=False) + 1]
        absent = next(v for v in range(1, T) if v not in roots)
        p = poly_from_roots(roots)
        for pos in sorted({0, c // 2, c}):
            rem = roots[:pos] + [absent] + roots[pos:]
            cnt, out, st = run(emu, p, rem, [7])
            assert cnt == -1 and st == (1, pos), (c, pos)
            assert all(v == 0xDEAD for v in out)
            assert divide(poly_from_roots(roots[pos:]), absent)[1] != 0


def test_removing_the_last_item_leaves_one(emu):
    expect(emu, poly_from_roots([99]), [99], [], [1])
    expect(emu, poly_from_roots([99, 5]), [5, 99], [], [1])
    rng = np.random.default_rng(4)
    roots = roots_for(rng, 129)
    expect(emu, poly_from_roots(roots), roots[::-1], [], [1])


def test_non_monic_polynomial(emu):
    rng = np.random.default_rng(5)
    for c in (0, 3, 64, 100):
        roots = roots_for(rng, c)
        for lead in (2, T - 1, 31337):
            p = poly_from_roots(roots, lead=lead)
            ins = roots_for(rng, 2)
            expect(emu, p, roots[:c // 2], ins, poly_from_roots(roots[c // 2:] + ins, lead=lead))
    # an irreducible factor (x^2 - nr, nr a non-residue) times linear factors: only those come out
    nr = next(a for a in range(2, T) if pow(a, (T - 1) // 2, T) == T - 1)
    irreducible = [(-nr) % T, 0, 1]                        # x^2 - nr
    def times(p, r):
        q = [0] * (len(p) + 1)
        for i, c in enumerate(p):
            q[i + 1] = (q[i + 1] + c) % T
            q[i] = (q[i] - r * c) % T
        return q
    p = times(times(irreducible, 11), 12)
    expect(emu, p, [12, 11], [], irreducible)
    cnt, out, st = run(emu, irreducible, [3], [])
    assert cnt == -1 and st[0] == 1


def test_zero_polynomial_is_not_a_bin_and_rows_bound_the_result(emu):
    cnt, out, st = run(emu, [0, 0, 0], [], [5])
    assert cnt == -1 and st[0] == 2
    cnt, out, st = run(emu, poly_from_roots([1, 2, 3]), [], [5], rows=4)
    assert cnt == -1 and st[0] == 3
    cnt, out, st = run(emu, poly_from_roots([1, 2, 3]), [1], [5], rows=4)
    assert cnt == 3 and out == poly_from_roots([2, 3, 5])


def test_unlift_on_both_sides_of_the_threshold(emu):
    """k_lift stores v < (t + 1) / 2 as it is and v + (q_0 - t) otherwise; SEAL's monomial shortcut stores any v as it is"""
    for t, q0 in ((T, (1 << 40) - 87), (65537, 2 * 65537 + 1), ((1 << 20) + 7, (1 << 56) - 5)):
        half = (t + 1) // 2
        for v in (0, 1, half - 1, half, half + 1, t - 1):
            stored = v if v < half else v + (q0 - t)
            assert stored < q0
            assert emu.emu_bin_unlift(stored, t, q0) == v
            assert emu.emu_bin_unlift(v, t, q0) == v        # the un-lifted monomial value
