"""CPU tier of the cuckoo hashing (apsu_amd/csrc/cuckoo.h through libapsu_he_hostemu.so) against the independent model
tests/cuckoo_model.py: the location functions' tables, the locations, the table rule and the database side's grouping."""
import ctypes as C

import numpy as np
import pytest

import cuckoo_cases
import cuckoo_model as M
import emu_lib


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def emu_locations(emu, items, H, T):
    items = np.ascontiguousarray(items, dtype=np.uint8).reshape(-1, 16)
    locs = np.zeros((len(items), H), dtype=np.uint32)
    assert emu.emu_cuckoo_locations(_vp(items), C.c_uint64(len(items)), C.c_uint32(H), C.c_uint32(T), _vp(locs)) == 0, emu.emu_last_error()
    return locs


def emu_insert(emu, items, locs, H, T, max_rounds):
    """-> (status, table_idx, item_loc, rounds, unplaced, placed)"""
    items = np.ascontiguousarray(items, dtype=np.uint8).reshape(-1, 16)
    locs = np.ascontiguousarray(locs, dtype=np.uint32)
    table_idx = np.zeros(T, dtype=np.uint32)
    item_loc = np.zeros(max(len(items), 1), dtype=np.uint32)
    rounds, unplaced, placed = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = emu.emu_cuckoo_insert(_vp(items), _vp(locs), C.c_uint64(len(items)), C.c_uint32(H), C.c_uint32(T), C.c_uint64(max_rounds), _vp(table_idx),
                               _vp(item_loc), C.byref(rounds), C.byref(unplaced), C.byref(placed))
    assert rc in (0, 1), emu.emu_last_error()
    return rc, table_idx, item_loc[:len(items)], rounds.value, unplaced.value, placed.value


def held_against_model(emu, case):
    name, items, locs, H, T, max_rounds, succeeds = case
    want = M.insert(list(items), locs.tolist(), H, T, max_rounds)
    assert want.ok == succeeds, name
    rc, table_idx, item_loc, rounds, unplaced, placed = emu_insert(emu, items, locs, H, T, max_rounds)
    assert rounds == want.rounds, name
    if not succeeds:
        assert rc == 1 and unplaced == want.unplaced and placed == round(want.fill * T), name
        return want
    assert rc == 0, name
    assert table_idx.tolist() == want.table_idx and item_loc.tolist() == want.item_loc, name
    M.check_invariants(list(items), locs.tolist(), want)
    return want


@pytest.mark.parametrize("f", [0, 1, 7])
def test_tables_equal_the_model(emu, f):
    tab = np.zeros((16, 256), dtype=np.uint32)
    emu.emu_cuckoo_tables(C.c_uint32(f), _vp(tab))
    assert tab.tolist() == [list(row) for row in M.tables(f)]
    assert len(set(tab.reshape(-1).tolist())) > 4000                    # (not a constant, not a short cycle)


def edge_items():
    rng = np.random.default_rng(0x4C4F43)
    base = rng.integers(1, 255, 16, dtype=np.uint8)
    rows = [np.zeros(16, dtype=np.uint8), np.full(16, 255, dtype=np.uint8), base]
    for p in range(16):                                                # 0x00 and 0xFF in every byte position, and one-byte neighbours
        for v in (0x00, 0xFF, int(base[p]) ^ 1):
            it = base.copy()
            it[p] = v
            rows.append(it)
    return np.array(rows, dtype=np.uint8)


@pytest.mark.parametrize("T", [1, 409, 6552, 1 << 30])
@pytest.mark.parametrize("H", [1, 3, 8])
def test_locations_equal_the_model(emu, H, T):
    items = edge_items()
    got = emu_locations(emu, items, H, T)
    assert got.tolist() == M.locations([bytes(it) for it in items], H, T)
    assert (got < T).all()
    if T == 1 << 30:
        # items that differ in one byte differ in that byte's table word alone, and function f does not depend on H
        assert len({tuple(r) for r in got.tolist()}) == len(items)
        assert (emu_locations(emu, items, 8, T)[:, :H] == got).all()


def test_collision_cases_equal_the_model(emu):
    for case in cuckoo_cases.collision_cases():
        held_against_model(emu, case)


def test_eviction_chain_is_the_one_built_by_hand(emu):
    case = [c for c in cuckoo_cases.collision_cases() if c[0] == "eviction chain"][0]
    want = held_against_model(emu, case)
    assert want.rounds == 4 and want.item_loc == [0, 2, 3, 4] and want.table_idx == [0, M.NONE, 1, 2, 3]


def test_failure_names_the_lowest_unplaced_item_and_stops(emu):
    case = [c for c in cuckoo_cases.collision_cases() if c[0] == "three items on two locations"][0]
    _, items, locs, H, T, max_rounds, _ = case
    rc, _, _, rounds, unplaced, placed = emu_insert(emu, items, locs, H, T, max_rounds)
    assert rc == 1 and rounds == 16 and unplaced in (0, 1, 2) and placed == 2
    assert unplaced == M.insert(list(items), locs.tolist(), H, T, max_rounds).unplaced


def test_duplicates_keep_the_lowest_index(emu):
    for name in ("adjacent duplicates", "duplicates far apart", "a triple", "duplicate of an item evicted later"):
        case = [c for c in cuckoo_cases.collision_cases() if c[0] == name][0]
        want = held_against_model(emu, case)
        items = [bytes(it) for it in case[1]]
        for i, loc in enumerate(want.item_loc):
            assert (loc == M.NONE) == (items[i] in items[:i]), name


def test_rounds_outside_the_key_are_refused(emu):
    items = np.zeros((1, 16), dtype=np.uint8)
    locs = np.zeros((1, 1), dtype=np.uint32)
    out = np.zeros(4, dtype=np.uint32)
    w = [C.c_uint64() for _ in range(3)]
    for bad in (0, (1 << 32) + 1):
        assert emu.emu_cuckoo_insert(_vp(items), _vp(locs), C.c_uint64(1), C.c_uint32(1), C.c_uint32(1), C.c_uint64(bad), _vp(out), _vp(out),
                                     C.byref(w[0]), C.byref(w[1]), C.byref(w[2])) == -1
    assert emu_insert(emu, items, locs, 1, 1, 1 << 32)[0] == 0


@pytest.mark.parametrize("pair", M.shipped_pairs(), ids=lambda p: "%d-in-%d-H%d" % p)
def test_shipped_pairs_equal_the_model(emu, pair):
    """every shipped (set size, table_size, hash_func_count) once, random items under a fixed seed, the real location functions"""
    size, T, H = pair
    rng = np.random.default_rng(0x53484950 + size * 7 + T)
    items = rng.integers(0, 256, (size, 16), dtype=np.uint8)
    locs = emu_locations(emu, items, H, T)
    if size <= 2048:                                                    # (the locations of the large sets are held against the model by sample)
        assert locs.tolist() == M.locations([bytes(it) for it in items], H, T)
    else:
        pick = rng.choice(size, 256, replace=False)
        assert locs[pick].tolist() == M.locations([bytes(it) for it in items[pick]], H, T)
    want = M.insert(list(items), locs.tolist(), H, T)
    assert want.ok and want.rounds <= 500                               # the precondition: the model alone finishes
    rc, table_idx, item_loc, rounds, _, _ = emu_insert(emu, items, locs, H, T, 500)
    assert rc == 0 and rounds == want.rounds
    assert table_idx.tolist() == want.table_idx and item_loc.tolist() == want.item_loc
    M.check_invariants(list(items), locs.tolist(), want)


def emu_bucket(emu, locs, T):
    locs = np.ascontiguousarray(locs, dtype=np.uint32)
    count, H = locs.shape
    offsets = np.zeros(T + 1, dtype=np.uint64)
    order = np.full(max(count * H, 1), 0xFFFFFFFF, dtype=np.uint32)
    total = C.c_uint64()
    rc = emu.emu_bucket_items(_vp(locs), C.c_uint64(count), C.c_uint32(H), C.c_uint32(T), _vp(offsets), _vp(order), C.byref(total))
    return rc, offsets, order, total.value


def test_bucket_items_is_stable_and_collapses_self_collisions(emu):
    locs = np.array([[4, 1, 4], [1, 1, 1], [0, 4, 2], [4, 2, 1], [2, 0, 0]], dtype=np.uint32)
    rc, offsets, order, total = emu_bucket(emu, locs, 6)
    assert rc == 0
    assert offsets.tolist() == [0, 2, 5, 8, 8, 11, 11] and total == 11 == offsets[6]
    assert order[:total].tolist() == [2, 4, 0, 1, 3, 2, 3, 4, 0, 2, 3]   # input order inside every bucket, item 1 once in bucket 1
    assert (order[total:] == 0xFFFFFFFF).all()                          # nothing behind the total is written
    want_off, want_order = M.bucket(locs.tolist(), 6)
    assert offsets.tolist() == want_off and order[:total].tolist() == want_order


def test_bucket_items_equals_the_model_on_random_locations(emu):
    rng = np.random.default_rng(7)
    for count, H, T in ((0, 3, 5), (1, 1, 1), (500, 3, 64), (300, 8, 7)):
        locs = rng.integers(0, T, (count, H)).astype(np.uint32)
        rc, offsets, order, total = emu_bucket(emu, locs, T)
        want_off, want_order = M.bucket(locs.tolist(), T)
        assert rc == 0 and offsets.tolist() == want_off and total == want_off[T] and order[:total].tolist() == want_order
    assert emu_bucket(emu, np.array([[0, 5, 1]], dtype=np.uint32), 5)[0] == -1   # a location outside the table


def test_query_values_layout_and_padding(emu):
    """slot b * items_per_bundle + k fills positions k F .. k F + F - 1 of row b with the item's bit split, zeros up to n"""
    rng = np.random.default_rng(11)
    nb, ipb, F, bpf, n = 3, 9, 7, 15, 64
    bits = F * bpf
    items = rng.integers(0, 256, (nb * ipb, 16), dtype=np.uint8)
    values = np.full((nb, n), 0xFFFF, dtype=np.uint64)
    emu.emu_query_values(_vp(items), C.c_uint32(nb), C.c_uint32(ipb), C.c_uint32(F), C.c_uint32(bpf), C.c_uint32(bits), C.c_uint64(n), _vp(values))
    for b in range(nb):
        for k in range(ipb):
            v = int.from_bytes(bytes(items[b * ipb + k]), "little") & ((1 << bits) - 1)
            assert values[b, k * F:(k + 1) * F].tolist() == [(v >> (j * bpf)) & ((1 << bpf) - 1) for j in range(F)]
        assert (values[b, ipb * F:] == 0).all()
