"""CPU tier of reading a BinBundle's bins back (apsu_amd/csrc/bin_roots.h): the field generator, the coset walk, the point table and
the lane functions of k_bin_roots / k_roots_mult, stepped over the lanes of a workgroup by the CPU emulation library (emu_bin_roots,
which runs the workgroup transform's own pass functions through the SrcCoset load) and held to Python's big integers.  All comparisons
are exact."""
import ctypes as C
import glob
import json
import os

import numpy as np
import pytest

import emu_lib
from emu_lib import vp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [(7681, 6), (769, 6), (257, 6), (12289, 8)]          # (t, log2 n) with t = 1 (mod 2n): 120, 12, 4 and 48 cosets
# (a ring of 32 slots has no workgroup transform form, so (193, 32) cannot be run through the lanes; (257, 64) takes its place)


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


def prime_factors(m):
    out, p = [], 2
    while p * p <= m:
        if m % p == 0:
            out.append(p)
            while m % p == 0:
                m //= p
        p += 1
    if m > 1:
        out.append(m)
    return out


def smallest_generator(t):
    ps = prime_factors(t - 1)
    return next(g for g in range(2, t) if all(pow(g, (t - 1) // p, t) != 1 for p in ps))


def is_prime(p):
    return p >= 2 and all(p % d for d in range(2, int(p ** 0.5) + 1))


def batching_prime(n, bits):
    """SEAL's PlainModulus::Batching: the largest prime below 2^bits that is 1 (mod 2n)"""
    p = (1 << bits) - 2 * n + 1
    while not is_prime(p):
        p -= 2 * n
    return p


def shipped_params():
    out = []
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "params", "*.json"))):
        with open(path) as f:
            sp = json.load(f)["seal_params"]
        n = int(sp["poly_modulus_degree"])
        t = int(sp["plain_modulus"]) if "plain_modulus" in sp else batching_prime(n, int(sp["plain_modulus_bits"]))
        out.append((os.path.basename(path), t, n))
    return out


def poly_from_roots(roots, t):
    p = [1]
    for r in roots:
        q = [0] * (len(p) + 1)
        for i, a in enumerate(p):
            q[i + 1] = (q[i + 1] + a) % t
            q[i] = (q[i] - r * a) % t
        p = q
    return p                                              # p[i] = coefficient of x^i, monic


def poly_mul(a, b, t):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % t
    return out


def run_bin(emu, t, logn, coeffs, blocks=1, rows=None):
    """-> (values, mult) in the order found, through the lanes"""
    rows = rows or len(coeffs)
    col = np.zeros(rows, dtype=np.uint64)
    col[:len(coeffs)] = coeffs
    cap = max(rows, 1)
    values, mult = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32)
    found = emu.emu_bin_roots(logn, C.c_uint64(t), vp(col), rows, blocks, vp(values), vp(mult), cap)
    assert found >= 0, emu.emu_last_error().decode()
    return values[:found], mult[:found]


def expand(emu, slot, count, values, mult):
    out = np.zeros(max(count, 1), dtype=np.uint64)
    rc = emu.emu_roots_expand(slot, count, vp(values), vp(mult), len(values), vp(out))
    return (out[:count].tolist(), None) if rc == 0 else (None, emu.emu_last_error().decode())


def bins_back(emu, t, logn, roots, blocks=1):
    coeffs = poly_from_roots(roots, t)
    values, mult = run_bin(emu, t, logn, coeffs, blocks)
    got, err = expand(emu, 0, len(roots), values, mult)
    assert err is None, err
    return got


def test_shipped_files_are_all_there():
    assert len(shipped_params()) == 36


def test_generator_of_every_shipped_plain_modulus(emu):
    for name, t, _ in shipped_params():
        assert emu.emu_field_generator(C.c_uint64(t)) == smallest_generator(t), name


def test_generator_small_fields(emu):
    for t in (3, 5, 7, 193, 257, 769, 7681, 12289, 114689):
        assert emu.emu_field_generator(C.c_uint64(t)) == smallest_generator(t)


def test_coset_bound_over_all_shipped_files(emu):
    most = 0
    for name, t, n in shipped_params():
        assert (t - 1) % (2 * n) == 0, name
        got = emu.emu_roots_coset_count(C.c_uint64(t), C.c_uint64(n))
        assert got == (t - 1) // n, (name, emu.emu_last_error())
        assert got <= 65536
        most = max(most, got)
    assert most == 8184                                   # 256M-*: the 26-bit prime 8184 * 8192 + 1, just under 2^26 / 8192 = 8192


def test_coset_bound_refuses(emu):
    t33 = 4294967311                                      # not 1 (mod 128): refused as not batching
    assert emu.emu_roots_coset_count(C.c_uint64(t33), C.c_uint64(64)) == -1
    t = next(p for p in range((1 << 23) + 1, 1 << 24, 128) if all(p % d for d in range(3, 4100, 2)))   # a 24-bit prime = 1 (mod 128)
    assert emu.emu_roots_coset_count(C.c_uint64(t), C.c_uint64(64)) == -1
    msg = emu.emu_last_error().decode()
    assert str(t) in msg and str((t - 1) // 64) in msg
    assert emu.emu_roots_coset_count(C.c_uint64(65536 * 64 + 1), C.c_uint64(64)) == 65536   # the bound itself passes (the count is all that is asked here)


@pytest.mark.parametrize("t,logn", SMALL)
def test_walk_visits_every_unit_exactly_once(emu, t, logn):
    n = 1 << logn
    out = np.zeros((t - 1) // n * n, dtype=np.uint64)
    assert emu.emu_roots_walk(logn, C.c_uint64(t), vp(out)) == 0, emu.emu_last_error()
    assert sorted(out.tolist()) == list(range(1, t))


@pytest.mark.parametrize("t,logn", SMALL)
def test_point_table_against_direct_evaluation(emu, t, logn):
    """the transform of X names each output position's evaluation point: the transform of any polynomial holds its values there"""
    n = 1 << logn
    pts = np.zeros(n, dtype=np.uint64)
    assert emu.emu_roots_points(logn, C.c_uint64(t), vp(pts)) == 0
    assert len(set(pts.tolist())) == n and all(pow(int(x), n, t) == t - 1 for x in pts)      # the n roots of x^n + 1
    rng = np.random.default_rng(5)
    a = rng.integers(0, t, n).astype(np.uint64)
    y = a.copy()
    assert emu.emu_ntt_limb_c(logn, 0, C.c_uint64(t), vp(y), max(64, n // 16), 16) == 0
    for k in range(n):
        x, acc = int(pts[k]), 0
        for c in reversed(a.tolist()):
            acc = (acc * x + c) % t
        assert acc == int(y[k])


@pytest.mark.parametrize("t,logn", SMALL)
@pytest.mark.parametrize("blocks", [1, 3])
def test_known_multisets_come_back(emu, t, logn, blocks):
    n = 1 << logn
    rng = np.random.default_rng(t + blocks)
    simple = sorted(rng.choice(np.arange(1, t), size=min(20, n - 1), replace=False).tolist())
    cases = {
        "simple": simple,
        "double and triple": sorted([5, 5, 17, 17, 17, 99] + simple[:7]),
        "root 0 once": sorted([0] + simple[:5]),
        "root 0 twice": sorted([0, 0, 3, 3, t - 1]),
        "count 1": [t - 1],
        "count 1, the root 0": [0],
        "one value only": [5] * 9,
        "count n - 1": sorted(rng.integers(0, t, n - 1).tolist()),
    }
    for name, roots in cases.items():
        assert bins_back(emu, t, logn, roots, blocks) == roots, name


def test_more_than_one_wave_of_roots_with_a_late_multiple_root(emu):
    """n = 256: more than 64 distinct roots, so the multiplicity wave takes several rounds, and the divisions of one round are seen by the next"""
    t, logn = 12289, 8
    rng = np.random.default_rng(11)
    distinct = rng.choice(np.arange(0, t), size=150, replace=False).tolist()
    roots = sorted(distinct + [distinct[3]] + [distinct[100]] * 2 + [distinct[149]])
    assert bins_back(emu, t, logn, roots, 5) == roots


def test_empty_bin_and_zero_polynomial(emu):
    t, logn = 7681, 6
    values, mult = run_bin(emu, t, logn, [1234], rows=4)            # count 0: a non-zero constant, no root
    assert len(values) == 0
    assert expand(emu, 7, 0, values, mult) == ([], None)
    col = np.zeros(4, dtype=np.uint64)
    out = np.zeros(4, dtype=np.uint64)
    m = np.zeros(4, dtype=np.uint32)
    assert emu.emu_bin_roots(logn, C.c_uint64(t), vp(col), 4, 1, vp(out), vp(m), 4) == -1
    assert "zero polynomial" in emu.emu_last_error().decode()


def test_non_split_polynomial_is_refused(emu):
    t, logn = 7681, 6
    nonres = next(a for a in range(2, t) if pow(a, (t - 1) // 2, t) == t - 1)
    irreducible = [(-nonres) % t, 0, 1]                   # x^2 - a, a no square
    coeffs = poly_mul(poly_from_roots([4, 4, 9], t), irreducible, t)
    values, mult = run_bin(emu, t, logn, coeffs, 2)
    assert sorted(zip(values.tolist(), mult.tolist())) == [(4, 2), (9, 1)]
    got, err = expand(emu, 41, 5, values, mult)
    assert got is None
    assert "bin 41" in err and "degree 5" in err and "does not split" in err and "3 roots" in err


def test_sum_check_has_teeth(emu):
    """hand-built wrong answers from the device side are refused by the host end, whatever is wrong with them"""
    values = np.array([3, 8, 20], dtype=np.uint64)
    ok = np.array([1, 2, 1], dtype=np.uint32)
    assert expand(emu, 0, 4, values, ok) == ([3, 8, 8, 20], None)
    for count, mult in ((4, [1, 1, 1]), (4, [1, 3, 1]), (4, [0, 2, 1]), (2, [1, 1, 1]), (5, [1, 2, 1])):
        got, err = expand(emu, 9, count, values, np.array(mult, dtype=np.uint32))
        assert got is None and "bin 9" in err and "does not split" in err


def test_random_bins_at_a_shipped_ring_size(emu):
    """n = 4096 with a small plain modulus (40961 = 5 * 8192 + 1: ten cosets): the transform form the shipped sets run"""
    t, logn = 40961, 12
    rng = np.random.default_rng(3)
    roots = sorted(rng.integers(0, t, 60).tolist() + [0, 0, 77, 77, 77])
    assert bins_back(emu, t, logn, roots, 4) == roots
