"""CPU tier of the plaintext answer of a BinBundle: k_bins_eval as the waves run it (apsu_amd/csrc/bin_eval.h: lane = slot, the tile's
top from the counts, EVAL_ROWS rows in flight, one Horner step per row in the width the plain modulus takes) stepped lane by lane by the
CPU emulation library (emu_bins_eval) and held to Python-integer Horner evaluation; and the reduction of self-test reports
(self_test_reduce through emu_self_test_reduce).  All comparisons are exact integers."""
import ctypes as C
import glob
import json
import os
import subprocess

import numpy as np
import pytest

import emu_lib
from emu_lib import vp
from test_bundle_merge_cpu import T32, T33, T60, is_prime, param_moduli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 128                                                   # two tiles of 64 slots
TABLE = (40961, 65537, 1032193, T32, T33, T60)            # the issue's list: three batching primes, either side of 2^32, 60 bits


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


def all_moduli():
    return sorted(set(TABLE) | set(param_moduli()))


def max_items():
    """the largest max_items_per_bin of the shipped parameter files"""
    most = 0
    for path in glob.glob(os.path.join(ROOT, "tests", "params", "*.json")):
        with open(path) as f:
            most = max(most, int(json.load(f)["table_params"]["max_items_per_bin"]))
    return most


def horner(col, x, t):
    acc = 0
    for c in reversed(col):
        acc = (acc * x + int(c)) % t
    return acc


def model(t, A, x, mask):
    n = A.shape[1]
    out, is_bin = [], []
    for s in range(n):
        col = [int(v) for v in A[:, s]]
        out.append((horner(col, int(x[s]), t) + (int(mask[s]) if mask is not None else 0)) % t)
        is_bin.append(int(any(col)))
    return out, is_bin


def run(emu, t, A, x, mask, wide=0):
    A = np.ascontiguousarray(A, dtype=np.uint64)
    rows, n = A.shape
    x = np.ascontiguousarray(x, dtype=np.uint64)
    m = np.ascontiguousarray(mask, dtype=np.uint64) if mask is not None else None
    out = np.full(n, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    is_bin = np.full(n, 0xEE, dtype=np.uint8)
    walked = np.zeros((n + 63) // 64, dtype=np.uint32)
    rc = emu.emu_bins_eval(C.c_uint64(t), vp(A), C.c_uint64(n), C.c_uint32(rows), vp(x), vp(m) if m is not None else None, C.c_int(wide), vp(out),
                           vp(is_bin), vp(walked))
    assert rc == 0, emu.emu_last_error()
    return [int(v) for v in out], [int(v) for v in is_bin], [int(v) for v in walked]


def check(emu, t, A, x, mask):
    want = model(t, A, x, mask)
    got = run(emu, t, A, x, mask)
    assert (got[0], got[1]) == want
    if t < 2 ** 32:                                       # the 128-bit step agrees wherever both are exact
        assert run(emu, t, A, x, mask, wide=1)[:2] == want
    return got[2]


def shape_degrees(emu):
    r = emu.emu_eval_rows()
    return sorted({0, 1, r - 1, r, r + 1})


def test_the_table_holds_what_it_says():
    assert T32 < 2 ** 32 < T33 and T60.bit_length() == 60
    assert all(is_prime(t) for t in TABLE)
    assert {40961, 65537, 1032193} <= set(all_moduli()) and len(param_moduli()) >= 1


@pytest.mark.parametrize("t", all_moduli())
def test_worst_case_coefficients_and_points(emu, t):
    """every coefficient t - 1 at the points 0, 1, t - 1 and a random one, masks 0 .. t - 1: the largest sums either width meets"""
    rng = np.random.default_rng(t % 1000)
    for deg in shape_degrees(emu):
        A = np.full((deg + 1, N), t - 1, dtype=np.uint64)
        x = np.array([(0, 1, t - 1, int(rng.integers(0, t)))[s % 4] for s in range(N)], dtype=np.uint64)
        mask = np.array([(t - 1, 0, 1, int(rng.integers(0, t)))[(s // 4) % 4] for s in range(N)], dtype=np.uint64)
        assert check(emu, t, A, x, mask) == [deg + 1, deg + 1]
        check(emu, t, A, x, None)


@pytest.mark.parametrize("t", all_moduli())
def test_random_polynomials_of_every_walk_shape(emu, t):
    rng = np.random.default_rng(7)
    for deg in shape_degrees(emu):
        A = rng.integers(0, t, (deg + 1, N), dtype=np.uint64)
        A[deg, :] = 1                                     # monic, as the bins' polynomials are
        x = rng.integers(0, t, N, dtype=np.uint64)
        mask = rng.integers(0, t, N, dtype=np.uint64)
        check(emu, t, A, x, mask)


@pytest.mark.parametrize("t", (65537, T33, T60))
def test_the_tallest_bin_a_parameter_file_allows(emu, t):
    deg = max_items() - 1
    assert deg >= 1000                                    # 16M-4096: 1304 items per bin
    n = 64
    A = np.full((deg + 1, n), t - 1, dtype=np.uint64)
    x = np.array([(0, 1, t - 1, 2)[s % 4] for s in range(n)], dtype=np.uint64)
    x[4:8] = [t - 2, 3, t // 2, t // 2 + 1]
    assert check(emu, t, A, x, np.full(n, t - 1, dtype=np.uint64)) == [deg + 1]


@pytest.mark.parametrize("t", (40961, T33))
def test_zero_polynomial_empty_bin_and_a_short_tile(emu, t):
    """slot 0 holds the zero polynomial (mask alone, not a bin), slot 1 the polynomial 1 of an empty bin (1 + mask); the second tile's
    largest count is 2 in an array of 12 rows, and a third tile has no bin at all"""
    rng = np.random.default_rng(3)
    n, rows = 192, 12
    A = np.zeros((rows, n), dtype=np.uint64)
    A[:, 2:64] = rng.integers(0, t, (rows, 62), dtype=np.uint64)
    A[rows - 1, 2:64] = 1
    A[0, 1] = 1
    A[:3, 64:128] = rng.integers(0, t, (3, 64), dtype=np.uint64)
    A[2, 64:128] = 1
    x = rng.integers(0, t, n, dtype=np.uint64)
    mask = rng.integers(0, t, n, dtype=np.uint64)
    out, is_bin, walked = run(emu, t, A, x, mask)
    assert (out, is_bin) == model(t, A, x, mask)
    assert out[0] == int(mask[0]) and is_bin[0] == 0
    assert out[1] == (1 + int(mask[1])) % t and is_bin[1] == 1
    assert walked == [rows, 3, 0]
    assert out[128:] == [int(v) for v in mask[128:]] and not any(is_bin[128:])
    assert run(emu, t, A, x, None)[0][128:] == [0] * 64


def test_a_value_that_is_not_reduced_is_refused(emu):
    t = 40961
    A = np.ones((1, 64), dtype=np.uint64)
    x = np.zeros(64, dtype=np.uint64)
    out = np.zeros(64, dtype=np.uint64)
    bad = x.copy()
    bad[5] = t
    assert emu.emu_bins_eval(C.c_uint64(t), vp(A), C.c_uint64(64), C.c_uint32(1), vp(bad), None, 0, vp(out), None, None) == -1
    assert emu.emu_bins_eval(C.c_uint64(t), vp(A), C.c_uint64(64), C.c_uint32(1), vp(x), vp(bad), 0, vp(out), None, None) == -1
    assert b"not reduced" in emu.emu_last_error()


# ------------------------------------------------------------------------------------------------------- the reports' reduction
class Report(C.Structure):
    _fields_ = [("bundles", C.c_uint32), ("reserved", C.c_uint32), ("slots", C.c_uint64), ("mismatches", C.c_uint64),
                ("first_bundle", C.c_int32), ("first_slot", C.c_uint32), ("first_got", C.c_uint64), ("first_expected", C.c_uint64),
                ("min_budget_bits", C.c_int32), ("min_budget_bundle", C.c_int32), ("he_ms", C.c_double), ("plain_ms", C.c_double)]


def reduce_reports(emu, parts):
    assert emu.emu_self_test_report_bytes() == C.sizeof(Report)
    arr = (Report * len(parts))(*parts)
    out = Report()
    emu.emu_self_test_reduce(arr, len(parts), C.byref(out))
    return out


def test_reports_reduce_to_the_report_of_the_whole(emu):
    none = reduce_reports(emu, [])
    assert (none.bundles, none.slots, none.mismatches, none.first_bundle, none.min_budget_bundle) == (0, 0, 0, -1, -1)
    a = Report(2, 0, 128, 0, -1, 0, 0, 0, 9, 3, 1.5, 0.25)
    b = Report(3, 0, 192, 5, 4, 17, 11, 12, 9, 1, 1.0, 0.5)
    c = Report(1, 0, 64, 2, 2, 40, 21, 22, 12, 2, 0.5, 0.125)
    idle = Report(0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0.0, 0.0)              # a device that owns nothing
    for order in ([a, b, c, idle], [idle, c, b, a], [b, idle, a, c]):
        r = reduce_reports(emu, order)
        assert (r.bundles, r.slots, r.mismatches) == (6, 384, 7)
        assert (r.first_bundle, r.first_slot, r.first_got, r.first_expected) == (2, 40, 21, 22)
        assert (r.min_budget_bits, r.min_budget_bundle) == (9, 1)         # the smallest budget, at the lowest position that has it
        assert (r.he_ms, r.plain_ms) == (1.5, 0.5)
    d = Report(1, 0, 64, 1, 2, 39, 1, 2, 0, 0, 0.0, 0.0)                 # same BinBundle, lower slot; a budget of 0 bits counts
    r = reduce_reports(emu, [c, d])
    assert (r.first_bundle, r.first_slot, r.min_budget_bits, r.min_budget_bundle) == (2, 39, 0, 0)


# --------------------------------------------------------------------------------------------- sanitizers: a stand-alone program
def test_lane_functions_and_report_reduction_under_asan_ubsan(tmp_path):
    src = os.path.join(ROOT, "apsu_amd", "csrc")
    exe = str(tmp_path / "bin_eval_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", src,
                           os.path.join(ROOT, "tests", "native", "bin_eval_harness.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert r.stdout.strip().endswith("ok")
