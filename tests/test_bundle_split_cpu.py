"""CPU tier of splitting and moving resident BinBundles: the rules of apsu_amd/csrc/bin_split.h and db_rebase.h, and k_roots_split as its
workgroups run it (emu_roots_split steps the kernel's own functions over the work items), all through the CPU emulation library and held
to plain Python (tests/split_model.py: sorted() and slicing).  Every comparison is exact."""
import ctypes as C
import glob
import json
import os
import subprocess

import numpy as np
import pytest

import emu_lib
from emu_lib import vp
import split_model as M
from oracle import ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 65537


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


# --------------------------------------------------------------------------------------------- the rules
def test_split_cut_tiles_every_bin_evenly(emu):
    for c in range(0, 71):
        for k in range(1, max(c, 1) + 1):
            cuts = [emu.emu_split_cut(c, k, p) for p in range(k + 1)]
            assert cuts == [M.cut(c, k, p) for p in range(k + 1)]
            assert cuts[0] == 0 and cuts[-1] == c and all(a <= b for a, b in zip(cuts, cuts[1:]))      # the parts tile [0, c)
            sizes = [b - a for a, b in zip(cuts, cuts[1:])]
            assert max(sizes) - min(sizes) <= 1 and set(sizes) <= {c // k, -(-c // k)}
            for pos in range(c):
                p = emu.emu_split_part_of(c, k, pos)
                assert cuts[p] <= pos < cuts[p + 1]


def test_split_cut_with_more_parts_than_items(emu):
    for c in range(0, 9):
        for k in range(c + 1, 20):
            cuts = [emu.emu_split_cut(c, k, p) for p in range(k + 1)]
            sizes = [b - a for a, b in zip(cuts, cuts[1:])]
            assert cuts[0] == 0 and cuts[-1] == c and set(sizes) <= {0, 1}
            for pos in range(c):
                p = emu.emu_split_part_of(c, k, pos)
                assert cuts[p] <= pos < cuts[p + 1]


def test_split_parts_is_the_smallest_that_ends_below_the_limit(emu):
    for c in range(0, 71):
        for limit in range(2, 75):
            k = emu.emu_split_parts(c, limit)
            assert k == M.parts_needed(c, limit) and k >= 1
            assert -(-c // k) < limit                                 # every part takes insertions and can be exported
            assert k == 1 or -(-c // (k - 1)) >= limit                # and one part fewer would not do
    assert emu.emu_split_parts(0, 1) == 1
    assert emu.emu_split_parts(5, 1) == -1 and b"can be cut below" in emu.emu_last_error()
    assert emu.emu_split_parts(0, 0) == -1
    # the shipped pairs: a bin at the source's bound under the destination's
    assert emu.emu_split_parts(227, 128) == 2 and emu.emu_split_parts(50, 32) == 2 and emu.emu_split_parts(31, 51) == 1


def test_instances_follow_from_hstride(emu):
    for h, cap in ((1, 256), (256, 256), (257, 2048), (2048, 2048), (2049, 8192), (8192, 8192), (8193, 0)):
        assert emu.emu_split_capacity(h) == cap


# --------------------------------------------------------------------------------------------- the kernel, stepped
def run_emu(emu, case):
    hits, found, mult, occ = case.inputs()
    out = np.full(case.off[-1], M.POISON, dtype=np.uint64)
    counts_out = np.full((case.k, case.n), M.POISON32, dtype=np.uint32)      # (the launcher zeroes them)
    failure = np.array([M.NO_FAILURE], dtype=np.uint64)
    off = np.array(case.off[:-1], dtype=np.uint64)
    stride = np.array(case.stride, dtype=np.uint32)
    rc = emu.emu_roots_split(vp(hits), vp(found), vp(mult), C.c_uint32(case.hstride), vp(occ), vp(case.counts), C.c_uint32(len(case.bins)), C.c_uint32(case.k),
                             vp(out), vp(off), vp(stride), vp(counts_out), C.c_uint32(case.n), vp(failure))
    assert rc == 0, emu.emu_last_error()
    return out, counts_out, int(failure[0])


def check_case(got, case):
    want_out, want_counts, want_failure = case.expected()
    out, counts_out, failure = got
    assert failure == want_failure, case.name
    assert (counts_out == want_counts).all(), case.name
    assert (out == want_out).all(), case.name             # the parts' items, and poison wherever nothing may be written


@pytest.mark.parametrize("t", [T, 4294967291, 193])
def test_emu_roots_split_adversarial_lists(emu, t):
    cases = M.adversarial_cases(t)
    assert {c.k for c in cases} >= {1, 2, 3} and any(c.expected()[2] != M.NO_FAILURE for c in cases)
    for case in cases:
        check_case(run_emu(emu, case), case)


def test_emu_roots_split_reports_the_first_failing_slot(emu):
    case = next(c for c in M.adversarial_cases(T) if c.name == "total-below")
    _, counts_out, failure = run_emu(emu, case)
    assert failure == (3 << 32 | 3)                        # slot 3 before slot 20, three roots counted with multiplicity
    assert counts_out[:, 3].tolist() == [0, 0] and counts_out[:, 8].tolist() == [3, 3]
    case = next(c for c in M.adversarial_cases(T) if c.name == "found-above")
    assert run_emu(emu, case)[2] == (40 << 32 | 5)


def test_emu_roots_split_instance_boundaries(emu):
    for case in M.boundary_cases(T):
        assert emu.emu_split_capacity(case.hstride) in M.CAPS
        check_case(run_emu(emu, case), case)


def test_emu_roots_split_refuses_what_the_launcher_refuses(emu):
    case = M.adversarial_cases(T)[0]
    hits, found, mult, occ = case.inputs()
    z = np.zeros(4, dtype=np.uint64)
    for h, k in ((8193, 2), (40, 0)):
        rc = emu.emu_roots_split(vp(hits), vp(found), vp(mult), C.c_uint32(h), vp(occ), vp(case.counts), C.c_uint32(0), C.c_uint32(k), vp(z), vp(z), vp(z), vp(z),
                                 C.c_uint32(0), vp(z))
        assert rc == -1


# --------------------------------------------------------------------------------------------- moving: which parameter sets, and the plan
FIELDS = (("poly_modulus_degree", lambda p: p["seal_params"]["poly_modulus_degree"]), ("plain_modulus", None),
          ("felts_per_item", lambda p: p["item_params"]["felts_per_item"]), ("table_size", lambda p: p["table_params"]["table_size"]),
          ("hash_func_count", lambda p: p["table_params"]["hash_func_count"]))


_RESOLVED = {}


def plain_modulus(p):
    """the modulus itself: a file may give plain_modulus_bits, from which the ring size decides it"""
    q = ref.load_params(json.dumps(p))
    key = (q["n"], q["plain_modulus"], q["plain_bits"])
    if key not in _RESOLVED:
        _RESOLVED[key] = int(ref.RefContext.from_params(q).t)
    return _RESOLVED[key]


def test_rebase_compatible_over_all_pairs_of_shipped_parameters(emu):
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "params", "*.json")))
    assert len(files) == 36
    text = {os.path.basename(f)[:-5]: open(f).read() for f in files}
    parsed = {k: json.loads(v) for k, v in text.items()}
    key = {k: [plain_modulus(p) if get is None else get(p) for _, get in FIELDS] for k, p in parsed.items()}
    moved = set()
    for a in text:
        for b in text:
            rc = emu.emu_rebase_compatible(text[a].encode(), text[b].encode())
            why = emu.emu_last_error().decode()
            diff = [name for (name, _), x, y in zip(FIELDS, key[a], key[b]) if x != y]
            assert rc == (0 if diff else 1), (a, b, why)
            if diff:
                assert why.startswith(diff[0] + " differs"), (a, b, why)       # the first differing field, by name
            else:
                assert why == ""
                if parsed[a] != parsed[b]:
                    moved.add((a, b))
    assert {("256K-2048-cmp", "256K-2048-com"), ("256K-2048-com", "256K-2048-cmp"), ("1M-512-cmp", "1M-512-com"), ("1M-512-com", "1M-512-cmp")} <= moved


def plan(emu, max_count, bundle_idx, dst_max):
    nb = len(max_count)
    mc, bi = np.array(max_count, dtype=np.uint32), np.array(bundle_idx, dtype=np.uint32)
    parts, first = np.zeros(nb, dtype=np.uint32), np.zeros(nb, dtype=np.uint32)
    cap = 4096
    cache, origin = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
    total = emu.emu_rebase_plan(vp(mc), vp(bi), C.c_uint32(nb), C.c_uint32(dst_max), vp(parts), vp(first), vp(cache), vp(origin), C.c_uint64(cap))
    assert total >= 0, emu.emu_last_error()
    return parts.tolist(), first.tolist(), cache[:total].tolist(), origin[:total].tolist()


def test_rebase_plan_numbers_the_parts_densely_per_bundle_index(emu):
    # bundle indices interleaved, a BinBundle without bins, one that needs three parts
    max_count = [227, 10, 0, 127, 128, 300, 5]
    bundle_idx = [4, 0, 4, 0, 4, 9, 0]
    parts, first, cache, origin = plan(emu, max_count, bundle_idx, 128)
    assert parts == [M.parts_needed(c, 128) for c in max_count] == [2, 1, 1, 1, 2, 3, 1]
    assert origin == [0, 0, 1, 2, 3, 4, 4, 5, 5, 5, 6]                 # input order kept, parts consecutive
    assert first == [0, 2, 3, 4, 5, 7, 10]
    per_index = {}
    for o, c in zip(origin, cache):
        per_index.setdefault(bundle_idx[o], []).append(c)
    assert per_index == {4: [0, 1, 2, 3, 4], 0: [0, 1, 2], 9: [0, 1, 2]}      # dense per bundle index, by position
    assert plan(emu, [], [], 16) == ([], [], [], [])
    mc = np.array([3], dtype=np.uint32)
    z = np.zeros(4, dtype=np.uint32)
    assert emu.emu_rebase_plan(vp(mc), vp(z), C.c_uint32(1), C.c_uint32(1), vp(z), vp(z), vp(z), vp(z), C.c_uint64(4)) == -1


# --------------------------------------------------------------------------------------------- sanitizers: a stand-alone program
def test_split_functions_under_asan_ubsan(tmp_path):
    src = os.path.join(ROOT, "apsu_amd", "csrc")
    exe = str(tmp_path / "bin_split_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", src,
                           os.path.join(ROOT, "tests", "native", "bin_split_harness.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert r.stdout.strip().endswith("ok")
