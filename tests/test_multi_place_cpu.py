"""CPU tier: the rules of a resident database behind the multi-device handle (apsu_amd/csrc/multi_place.h), through the emulation
library: where a new BinBundle goes (place_new_unit), every id after BinBundles were dropped, replaced, merged or appended
(registry_after), the cache order of a bundle index and the device a merge is made on.  Each is held against a Python restatement, and
place_new_unit against the partition rule of the C ABI; a stand-alone program runs the header under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/native/multi_place_harness.cpp)."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import emu_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "apsu_amd", "csrc")


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


def ptr(a):
    return C.c_void_p(a.ctypes.data)


# ---- the restatements -----------------------------------------------------------------------------------------------
def candidates(b, count, world):
    return [r for r in range(world) if r % count == b] if world >= count else [b % world]


def model_place_new_unit(b, count, world, load):
    return min(candidates(b, count, world), key=lambda r: (load[r], r))


def model_registry_after(old, dropped, replaced, appended):
    """old / appended: (slot, bundle_idx, cache_idx, degree); dropped: bools; replaced: new degree or -1"""
    new_id, reg = [], []
    for u, d, r in zip(old, dropped, replaced):
        if d:
            new_id.append(-1)
            continue
        new_id.append(len(reg))
        reg.append(u if r < 0 else (u[0], u[1], u[2], r))
    for a in appended:
        new_id.append(len(reg))
        reg.append(a)
    return new_id, reg


def emu_place(emu, b, count, world, load):
    la = np.array(list(load) + [0], dtype=np.uint64)
    return emu.emu_place_new_unit(C.c_uint32(b), C.c_uint32(count), int(world), ptr(la))


def cols(units):
    """[(slot, bundle_idx, cache_idx, degree)] -> the four arrays (never empty, so that their pointers are valid)"""
    u = list(units) or [(0, 0, 0, 0)]
    return (np.array([x[0] for x in u], dtype=np.int32), np.array([x[1] for x in u], dtype=np.uint32),
            np.array([x[2] for x in u], dtype=np.uint32), np.array([x[3] for x in u], dtype=np.uint32))


def emu_registry_after(emu, old, dropped, replaced, appended):
    o, a = cols(old), cols(appended)
    dr = np.array(list(dropped) + [0], dtype=np.uint8)
    rp = np.array(list(replaced) + [-1], dtype=np.int64)
    cap = len(old) + len(appended) + 1
    new_id = np.full(cap, -7, dtype=np.int32)
    out = (np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32))
    k = emu.emu_registry_after(*[ptr(x) for x in o], len(old), ptr(dr), ptr(rp), *[ptr(x) for x in a], len(appended), ptr(new_id),
                               *[ptr(x) for x in out])
    if k < 0:
        return None, emu.emu_last_error().decode()
    assert int(new_id[cap - 1]) == -7                              # nothing written behind old + appended
    reg = [tuple(int(c[i]) for c in out) for i in range(k)]
    return [int(v) for v in new_id[:cap - 1]], reg


def emu_merge_home(emu, members):
    """members: (slot, bundle_idx, cache_idx, degree) -> (home slot, position of the first member in cache order)"""
    c = cols(members)
    first = C.c_uint32(99)
    home = emu.emu_merge_home(ptr(c[0]), ptr(c[2]), len(members), C.byref(first))
    return home, first.value


# ---- place_new_unit -------------------------------------------------------------------------------------------------
def test_place_new_unit_matches_the_restatement_for_every_world_and_index_count(emu):
    rng = np.random.default_rng(141)
    for world in range(1, 9):
        for count in range(1, 6):
            for b in range(count):
                for _ in range(20):
                    load = [int(v) for v in rng.integers(0, 5000, world)]
                    got = emu_place(emu, b, count, world, load)
                    assert got == model_place_new_unit(b, count, world, load), (world, count, b, load)
                    assert got in candidates(b, count, world)


def test_place_new_unit_ties_go_to_the_lowest_slot(emu):
    assert emu_place(emu, 0, 2, 6, [7, 0, 7, 0, 7, 0]) == 0       # slots 0, 2, 4 tie
    assert emu_place(emu, 1, 2, 6, [0, 9, 0, 3, 0, 3]) == 3       # slots 3 and 5 tie below slot 1
    assert emu_place(emu, 0, 1, 4, [5, 5, 5, 5]) == 0
    assert emu_place(emu, 0, 1, 4, [5, 4, 4, 5]) == 1
    assert emu_place(emu, 2, 3, 2, [100, 0]) == 0                  # fewer devices than indices: the one slot 2 % 2, whatever it carries
    assert emu_place(emu, 1, 3, 2, [0, 10 ** 15]) == 1
    # loads above 2^32 and 2^63 compare as unsigned 64-bit numbers
    assert emu_place(emu, 0, 1, 2, [2 ** 63 + 5, 2 ** 63 + 4]) == 1
    assert emu_place(emu, 0, 1, 2, [2 ** 32, 2 ** 32 - 1]) == 1


def test_place_new_unit_refusals(emu):
    for b, count, world, text in ((0, 0, 2, "bundle_idx_count"), (3, 3, 2, "out of range"), (0, 2, 0, "no devices")):
        assert emu_place(emu, b, count, world, [0, 0]) == -1
        assert text in emu.emu_last_error().decode()


def test_units_fed_one_by_one_give_the_partition_rule_without_spill(emu):
    """the LPT property: bundle index by bundle index, degree descending then cache_idx ascending -> partition_units(set, cost 0)"""
    import apsu_amd
    rng = np.random.default_rng(142)
    for trial in range(60):
        count = int(rng.integers(1, 6))
        world = int(rng.integers(1, 9))
        units = []
        for b in range(count):
            k = int(rng.integers(0, 12))
            # few distinct degrees, so that ties (decided by cache_idx, then by the lowest slot) occur
            units += [(b, int(ci), int(rng.choice([0, 3, 170, 170, 1303, 1303, 4000]))) for ci in rng.permutation(40)[:k]]
        order = [int(i) for i in rng.permutation(len(units))]
        units = [units[i] for i in order]
        want = apsu_amd.partition_bundles(units, count, world, 0)
        load = [0] * world
        got = [None] * len(units)
        for b in range(count):
            mine = sorted((i for i, u in enumerate(units) if u[0] == b), key=lambda i: (-units[i][2], units[i][1]))
            for i in mine:
                got[i] = emu_place(emu, b, count, world, load)
                load[got[i]] += units[i][2] + 64
        assert got == want, (trial, count, world, units)
        # device_loads is the same sum
        out = np.zeros(world + 1, dtype=np.uint64)
        slots = np.array(got + [0], dtype=np.int32)
        deg = np.array([u[2] for u in units] + [0], dtype=np.uint32)
        assert emu.emu_device_loads(ptr(slots), ptr(deg), len(units), world, ptr(out)) == 0
        assert [int(v) for v in out[:world]] == load


# ---- index_in_cache_order, merge_home ---------------------------------------------------------------------------------
def test_cache_order_of_an_index_and_its_refusal(emu):
    rng = np.random.default_rng(143)
    for _ in range(50):
        k = int(rng.integers(0, 13))
        bidx = np.array([int(v) for v in rng.integers(0, 3, k)] + [0], dtype=np.uint32)
        cidx = np.array([int(v) for v in rng.permutation(30)[:k]] + [0], dtype=np.uint32)
        ids = np.full(k + 1, -5, dtype=np.int32)
        for which in range(3):
            got = emu.emu_index_in_cache_order(ptr(bidx), ptr(cidx), k, which, ptr(ids))
            want = sorted((i for i in range(k) if bidx[i] == which), key=lambda i: int(cidx[i]))
            assert got == len(want) and [int(v) for v in ids[:got]] == want
    # the same cache_idx in two bundle indices is fine; twice in one index is refused
    bidx = np.array([0, 1, 0, 1], dtype=np.uint32)
    cidx = np.array([4, 4, 2, 2], dtype=np.uint32)
    ids = np.zeros(4, dtype=np.int32)
    assert emu.emu_index_in_cache_order(ptr(bidx), ptr(cidx), 4, 0, ptr(ids)) == 2 and [int(v) for v in ids[:2]] == [2, 0]
    cidx[2] = 4
    assert emu.emu_index_in_cache_order(ptr(bidx), ptr(cidx), 4, 0, ptr(ids)) == -1
    assert "share cache_idx 4" in emu.emu_last_error().decode()
    assert emu.emu_index_in_cache_order(ptr(bidx), ptr(cidx), 4, 1, ptr(ids)) == 2


def test_merge_home_is_the_slot_of_the_first_member_in_cache_order(emu):
    assert emu_merge_home(emu, [(2, 0, 7, 1), (0, 0, 3, 1), (1, 0, 5, 1)]) == (0, 1)
    assert emu_merge_home(emu, [(4, 1, 0, 9), (0, 1, 1, 9)]) == (4, 0)
    assert emu_merge_home(emu, [(3, 0, 2, 1)]) == (3, 0)
    assert emu_merge_home(emu, [])[0] == -1 and "no members" in emu.emu_last_error().decode()
    rng = np.random.default_rng(144)
    for _ in range(100):
        k = int(rng.integers(1, 8))
        m = [(int(rng.integers(0, 5)), 0, int(c), 0) for c in rng.permutation(20)[:k]]
        first = min(range(k), key=lambda i: m[i][2])
        assert emu_merge_home(emu, m) == (m[first][0], first)


# ---- registry_after -------------------------------------------------------------------------------------------------
def random_registry(rng, k, world=3, indices=2):
    reg = []
    for i in range(k):
        reg.append((int(rng.integers(0, world)), int(rng.integers(0, indices)), i if rng.integers(0, 2) else 40 - i, int(rng.integers(0, 12))))
    return reg


def check_invariants(old, dropped, replaced, appended, new_id, reg):
    survivors = [i for i in range(len(old)) if not dropped[i]]
    assert [new_id[i] for i in survivors] == list(range(len(survivors)))                 # dense, relative order kept
    assert all(new_id[i] == -1 for i in range(len(old)) if dropped[i])
    assert new_id[len(old):] == list(range(len(survivors), len(survivors) + len(appended)))   # appended follow, in order
    assert len(reg) == len(survivors) + len(appended)
    for i in survivors:
        u, v = old[i], reg[new_id[i]]
        assert v[:3] == u[:3] and v[3] == (u[3] if replaced[i] < 0 else replaced[i])      # slot, index, cache_idx stay
    assert reg[len(survivors):] == list(appended)


def test_registry_after_every_combination_over_random_registries(emu):
    rng = np.random.default_rng(145)
    cases = 0
    for k in range(0, 13):
        for with_drop, with_replace, with_merge, with_append in itertools.product((0, 1), repeat=4):
            for _ in range(3):
                old = random_registry(rng, k)
                dropped, replaced = [0] * k, [-1] * k
                free = list(range(k))
                if with_merge:
                    by_index = {}
                    for i in free:
                        by_index.setdefault(old[i][1], []).append(i)
                    groups = [v for v in by_index.values() if len(v) >= 2]
                    if groups:
                        g = groups[int(rng.integers(0, len(groups)))]
                        g = [int(i) for i in rng.permutation(g)[:int(rng.integers(2, len(g) + 1))]]
                        home, first = emu_merge_home(emu, [old[i] for i in g])
                        assert home == old[g[first]][0]
                        for pos, i in enumerate(g):                 # the merge in registry_after's two words
                            if pos == first:
                                replaced[i] = int(rng.integers(0, 12))
                            else:
                                dropped[i] = 1
                            free.remove(i)
                for i in list(free):
                    if with_drop and rng.integers(0, 3) == 0:
                        dropped[i] = 1
                        free.remove(i)
                    elif with_replace and rng.integers(0, 3) == 0:
                        replaced[i] = int(rng.integers(0, 12))
                appended = [(int(rng.integers(0, 3)), int(rng.integers(0, 2)), 50 + j, int(rng.integers(0, 12)))
                            for j in range(int(rng.integers(1, 4)) if with_append else 0)]
                got = emu_registry_after(emu, old, dropped, replaced, appended)
                assert got == model_registry_after(old, dropped, replaced, appended), (old, dropped, replaced, appended)
                check_invariants(old, dropped, replaced, appended, *got)
                cases += 1
    assert cases == 13 * 16 * 3


def test_registry_after_special_cases(emu):
    rng = np.random.default_rng(146)
    old = random_registry(rng, 9)
    # nothing changes
    new_id, reg = emu_registry_after(emu, old, [0] * 9, [-1] * 9, [])
    assert new_id == list(range(9)) and reg == old
    # everything is dropped (with and without appended BinBundles)
    new_id, reg = emu_registry_after(emu, old, [1] * 9, [-1] * 9, [])
    assert new_id == [-1] * 9 and reg == []
    new_id, reg = emu_registry_after(emu, old, [1] * 9, [-1] * 9, [(2, 1, 0, 5), (0, 1, 1, 6)])
    assert new_id == [-1] * 9 + [0, 1] and reg == [(2, 1, 0, 5), (0, 1, 1, 6)]
    # an empty registry
    assert emu_registry_after(emu, [], [], [], []) == ([], [])
    assert emu_registry_after(emu, [], [], [], [(1, 0, 0, 3)]) == ([0], [(1, 0, 0, 3)])
    # a merged group whose first member in cache order has the highest id: the merged BinBundle takes THAT place, on ITS slot
    old = [(0, 0, 9, 4), (1, 1, 0, 7), (2, 0, 5, 3), (1, 0, 2, 2)]
    group = [0, 2, 3]
    home, first = emu_merge_home(emu, [old[i] for i in group])
    assert (home, group[first]) == (1, 3)
    dropped, replaced = [1, 0, 1, 0], [-1, -1, -1, 8]
    new_id, reg = emu_registry_after(emu, old, dropped, replaced, [])
    assert new_id == [-1, 0, -1, 1] and reg == [(1, 1, 0, 7), (1, 0, 2, 8)]
    # an id cannot be dropped and replaced at once
    got, err = emu_registry_after(emu, old, [1, 0, 0, 0], [5, -1, -1, -1], [])
    assert got is None and "both dropped and replaced" in err


# ---- the header under the sanitizers --------------------------------------------------------------------------------
def test_multi_place_header_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "multi_place_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-I", SRC, os.path.join(ROOT, "tests", "native", "multi_place_harness.cpp"), os.path.join(SRC, "sharding.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert r.stdout.strip().endswith("ok") and "registries" in r.stdout
