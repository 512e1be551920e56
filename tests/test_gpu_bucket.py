"""GPU tier: the database side's grouping by location on the device (kernels_bucket.hip; apsu_amd/csrc/bucket_plan.h) and the gather of
the entries.  (i) the grouping alone through apsu_he_debug_bucket_locs on the steered locations of tests/bucket_cases.py, at the least tile
and at the default, word for word against the existing emu_bucket_items (cuckoo_bucket); (ii) the public call apsu_he_items_bucket_device
against apsu_he_items_bucket, with host and device pointers; (iii) items to a resident database and a query against it.  Every comparison
is exact; nothing behind the total may be written."""
import ctypes as C

import numpy as np
import pytest

import apsu_amd
import bucket_cases
import common
import test_gpu_bulk_build as BB
import test_gpu_cuckoo as CK

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POISON = bucket_cases.POISON


@pytest.fixture(scope="module")
def toy():
    G = apsu_amd.HeContext(common.toy_json())
    yield G
    G.close()


def run(G, locs, T, tile):
    """-> (offsets, order with one word of room behind count * H, total); order and offsets come in poisoned"""
    count, H = locs.shape
    order = np.full(count * H + 1, POISON, dtype=np.uint32)
    offsets = np.full(T + 1, POISON, dtype=np.uint64)
    return G.debug_bucket_locs(locs, T, tile, order=order, offsets=offsets)


# ------------------------------------------------------------------------------------------------------------- the grouping alone
@pytest.mark.parametrize("tile", [bucket_cases.TILE_MIN, 0])
def test_steered_locations_equal_cuckoo_bucket(toy, tile):
    """count in {0, 1, 63, 64, 65} x H in {1, 3, 8} x T in {1, 2, 255, 256, 257, 65537}; entry counts of tile - 1, tile, tile + 1 and
    3 tiles + 1; one bucket, the last bucket, two buckets apart in the high digit; collisions inside the items; 5000 random items"""
    cases = [c for c in bucket_cases.all_cases() if c[3] == tile]
    assert len(cases) > 100
    for name, locs, T, _ in cases:
        want_off, want_order = bucket_cases.reference(locs, T, name)
        offsets, order, total = run(toy, locs, T, tile)
        assert total == len(want_order) and (offsets == want_off).all(), name
        assert (order[:total] == want_order).all(), name
        assert (order[total:] == POISON).all(), name


@pytest.mark.parametrize("tile", [bucket_cases.TILE_MIN, 0])
def test_one_bucket_keeps_the_input_order(toy, tile):
    """stability across lanes, waves and tiles without a reference: every entry in one bucket -> order = 0 .. count - 1"""
    edge = tile or bucket_cases.TILE_DEFAULT
    for T, loc in ((1, 0), (65537, 65536), (6552, 4000)):
        for count in (1, 63, 64, 65, edge - 1, edge, edge + 1, 3 * edge + 1):
            offsets, order, total = run(toy, np.full((count, 1), loc, dtype=np.uint32), T, tile)
            assert total == count and (order[:count] == np.arange(count)).all() and order[count] == POISON, (T, count)
            assert (offsets[:loc + 1] == 0).all() and (offsets[loc + 1:] == count).all()
    # every function of an item on one location: the item is listed once
    offsets, order, total = run(toy, np.full((edge + 1, 3), 2, dtype=np.uint32), 3, tile)
    assert total == edge + 1 and (order[:total] == np.arange(total)).all() and (order[total:] == POISON).all()
    assert offsets.tolist() == [0, 0, 0, total]


def test_two_runs_give_the_same_words(toy):
    """whatever the scheduling: the words are a function of the input (collisions, three passes, several tiles)"""
    rng = np.random.default_rng(77)
    locs = rng.integers(0, 65537, (3000, 3)).astype(np.uint32)
    locs[::7, 2] = locs[::7, 0]
    first = run(toy, locs, 65537, 256)
    for tile in (256, 256, 512, 0):
        again = run(toy, locs, 65537, tile)
        assert again[2] == first[2] < 9000 and (again[0] == first[0]).all() and (again[1] == first[1]).all()
    want_off, want_order = bucket_cases.reference(locs, 65537)
    assert (first[0] == want_off).all() and (first[1][:first[2]] == want_order).all() and (first[1][first[2]:] == POISON).all()


def test_whole_call_crosses_the_scans_step(toy):
    """3000 items under 3 functions in 256 slots at tile 256: 36 tiles x 256 digits = 9216 words for the pass's scan, which takes 8192 a
    step -- the carry and the second step's tail inside the whole call"""
    locs = np.random.default_rng(3000).integers(0, 256, (3000, 3)).astype(np.uint32)
    assert -(-locs.size // 256) * 256 == 9216 > 8192 and bucket_cases.digit_plan(256) == (8, [8])
    want_off, want_order = bucket_cases.reference(locs, 256)
    assert 8192 < len(want_order) <= 9000                                          # collisions inside an item drop a few entries
    offsets, order, total = run(toy, locs, 256, 256)
    assert total == len(want_order) and (offsets == want_off).all()
    assert (order[:total] == want_order).all() and (order[total:] == POISON).all()


def test_hook_refusals_write_nothing(toy):
    locs = np.array([[0, 1, 2], [2, 3, 1]], dtype=np.uint32)
    with pytest.raises(ValueError, match="location 4 is outside the table"):       # a location equal to T
        run(toy, locs, 3, 0)
    for bad_locs, T, tile in ((locs, 3, 0), (locs, 0, 0), (np.zeros((2, 9), dtype=np.uint32), 4, 0), (locs, 4, 255), (locs, 4, 100),
                              (locs, 4, (1 << 20) + 256)):
        count, H = bad_locs.shape
        order, offsets = np.full(count * H + 1, POISON, dtype=np.uint32), np.full(T + 1, POISON, dtype=np.uint64)
        with pytest.raises(ValueError):
            toy.debug_bucket_locs(bad_locs, T, tile, order=order, offsets=offsets)
        assert (order == POISON).all() and (offsets == POISON).all()
    offsets, order, total = run(toy, locs, 4, 0)                                  # the context goes on working
    assert total == 6 and offsets.tolist() == [0, 1, 3, 5, 6] and order[:6].tolist() == [0, 0, 1, 0, 1, 1]
    off0, order0, total0 = run(toy, locs[:0], 4, 0)                              # no item: zeros, nothing launched
    assert total0 == 0 and (off0 == 0).all() and (order0 == POISON).all()


# ------------------------------------------------------------------------------------------------------------- the public call
@pytest.fixture(scope="module")
def shipped():
    G = apsu_amd.HeContext(common.param_json("256K-512"))
    items = CK.random_items(4096, 4096)
    items[100] = items[7]                                                  # (a repeated item is listed twice: the database side does not dedupe)
    want = G.bucket_items(items)
    yield G, items, want
    G.close()


def test_public_call_equals_items_bucket(shipped):
    G, items, (want_off, want_order) = shipped
    T, H = G.table_size, G.hash_func_count
    assert (T, H) == (819, 3) and len(want_order) <= 4096 * 3
    offsets, order, entries, total = G.bucket_items_device(items)
    assert total == len(want_order) and (offsets == want_off).all() and (order == want_order).all()
    assert entries.shape == (total, 16) and (entries == items[want_order]).all()
    locs_ms, sort_ms, gather_ms = G.bucket_times()
    assert locs_ms > 0 and sort_ms > 0 and gather_ms > 0
    # the forms without order, without entries, without both
    o2, none, e2, t2 = G.bucket_items_device(items, order=False)
    assert none is None and t2 == total and (o2 == want_off).all() and (e2 == entries).all()
    o3, ord3, none, t3 = G.bucket_items_device(items, entries=False)
    assert none is None and t3 == total and (o3 == want_off).all() and (ord3 == want_order).all()
    o4, a, b, t4 = G.bucket_items_device(items, order=False, entries=False)
    assert a is None and b is None and t4 == total and (o4 == want_off).all()
    for count in (0, 1, 65):
        o5, ord5, e5, t5 = G.bucket_items_device(items[:count])
        w_off, w_order = G.bucket_items(items[:count])
        assert t5 == len(w_order) and (o5 == w_off).all() and (ord5 == w_order).all() and (e5 == items[:count][w_order]).all()


def test_device_pointers_give_the_same_words(shipped):
    G, items, (want_off, want_order) = shipped
    total, room = len(want_order), 4096 * 3
    d_items = torch.from_numpy(items).cuda()
    for shift in (0, 4, 8):                                                # entries at an address that is a multiple of 16, and two that are not
        d_order = torch.full((room + 1,), -1, dtype=torch.int32, device="cuda")
        d_entries = torch.full((room * 16 + 32,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()                                           # (the engine's stream does not wait for torch's)
        offsets, none_o, none_e, got_total = G.bucket_items_device(d_items.data_ptr(), count=4096, order=d_order.data_ptr(), entries=d_entries.data_ptr() + shift)
        assert none_o is None and none_e is None and got_total == total and (offsets == want_off).all()
        back = d_order.cpu().numpy().view(np.uint32)
        assert (back[:total] == want_order).all() and (back[total:] == 0xFFFFFFFF).all()          # nothing behind the total is written
        ent = d_entries.cpu().numpy()
        assert (ent[shift:shift + total * 16].reshape(total, 16) == items[want_order]).all()
        assert (ent[:shift] == 0xEE).all() and (ent[shift + total * 16:] == 0xEE).all()
    # items at an address that is not a multiple of 16 (the kernels load 16 bytes at once: the engine moves them)
    d_odd = torch.zeros(16 * 4096 + 4, dtype=torch.uint8, device="cuda")
    d_odd[4:] = d_items.reshape(-1)
    torch.cuda.synchronize()
    offsets, order, entries, got_total = G.bucket_items_device(d_odd.data_ptr() + 4, count=4096)
    assert got_total == total and (offsets == want_off).all() and (order == want_order).all() and (entries == items[want_order]).all()


def test_public_call_refusals(shipped):
    G, items, _ = shipped
    with pytest.raises(ValueError, match="32-bit index"):
        G.bucket_items_device(1 << 20, count=2**32 - 1, order=False, entries=False)      # (refused before the pointer is looked at)
    raw = apsu_amd.HeContext(n=G.n, coeff_modulus=G.q, plain_modulus=G.t)
    with pytest.raises(apsu_amd.ApsuHeError):                                  # a context without PSUParams has no table
        raw.bucket_items_device(items)
    offsets, total = np.zeros(820, dtype=np.uint64), C.c_uint64()
    rc = apsu_amd.load_library().apsu_he_items_bucket_device(raw.h, C.c_void_p(items.ctypes.data), C.c_size_t(2), 0, C.c_void_p(offsets.ctypes.data),
                                                             None, 0, None, 0, C.byref(total))
    assert rc == -2                                                            # APSU_HE_LOGIC_ERROR, as the other N1 calls refuse it
    raw.close()


# ------------------------------------------------------------------------------------------------------------- to a database and a query
def xor_oprf(entries, offsets):
    assert entries.shape == (int(offsets[-1]), 16)
    return entries ^ np.uint8(0x5A)


@pytest.mark.parametrize("table_mult", [1, 2])
def test_database_from_items_equals_the_host_route(table_mult):
    """the toy set of tests/test_gpu_bulk_build.py (12 locations per bundle index, at most 10 entries of a location per BinBundle): 150 items
    give every bundle index several BinBundles.  Images byte for byte."""
    G = BB.context(table_mult=table_mult)
    items = BB.rand_entries(np.random.default_rng(40 + table_mult), 150)
    offsets, order = G.bucket_items(items)
    want = BB.images(G, G.build_database(items[order], offsets))
    assert len(want) > G.bundle_idx_count
    assert BB.images(G, G.build_database_from_items(items)) == want
    want_x = BB.images(G, G.build_database(xor_oprf(items[order], offsets), offsets))
    assert want_x != want
    assert BB.images(G, G.build_database_from_items(items, oprf=xor_oprf)) == want_x
    with pytest.raises(ValueError, match="one entry per entry"):
        G.build_database_from_items(items, oprf=lambda e, o: e[:-1])
    assert G.build_database_from_items(items[:0]) == []
    G.close()


def test_query_against_a_database_built_from_items():
    """256K-512, the items and the query of tests/test_gpu_cuckoo.py's loopback (300 in the database; 128 asked, 64 of them in it; that
    test holds the model to show no cross-item false positive for this seed): the database comes from build_database_from_items, the
    querier's side is the same.  An occupied slot decrypts to the mask in all felts of its item, in some BinBundle, iff the item is in."""
    js = common.param_json("256K-512")
    G = apsu_amd.HeContext(js)
    T, F, n, ipb = G.table_size, G.felts_per_item, G.n, int(G.info.items_per_bundle)
    rng = np.random.default_rng(0x32353651)
    db = rng.integers(0, 256, (300, 16), dtype=np.uint8)
    query = np.concatenate([db[rng.choice(300, 64, replace=False)], rng.integers(0, 256, (64, 16), dtype=np.uint8)])
    in_db = np.arange(128) < 64
    bundles = G.build_database_from_items(db)
    offsets, order = G.bucket_items(db)
    assert BB.images(G, bundles) == BB.images(G, G.build_database(db[order], offsets)) and len(bundles) >= 1
    table_idx, item_loc, _ = G.cuckoo_table(query)
    table_items = np.zeros((T, 16), dtype=np.uint8)
    occ = np.nonzero(table_idx != 0xFFFFFFFF)[0]
    table_items[occ] = query[table_idx[occ]]
    S, L = G.source_power_count, G.first_chain_idx + 1
    d_vals = torch.zeros(n, dtype=torch.int64, device="cuda")
    cts = torch.zeros((S, 2, L, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()                                               # (the engine's stream does not wait for torch's)
    G.query_values(table_items, values=d_vals.data_ptr())
    sk = G.keygen(CK.SEED)
    _, _, rk = G.relin_keygen(sk, CK.SEED, want_host=False)
    G.query_create(sk, [0], d_vals.data_ptr(), cts.data_ptr(), seed=CK.SEED, values_on_device=True)
    pw = G.compute_powers([0], [[cts.data_ptr() + s * 2 * L * n * 8 for s in range(S)]], rk, on_device=True)
    mbuf = torch.empty(len(bundles) * n, dtype=torch.int64, device="cuda")
    mask_vals, _ = G.mask_generate(77, len(bundles), mbuf.data_ptr(), want_blocks=False)
    out = torch.empty((len(bundles), 2, n), dtype=torch.int64, device="cuda")
    G.eval_bundles(bundles, pw, rk, [mbuf.data_ptr() + i * n * 8 for i in range(len(bundles))], out=out.data_ptr(), masks_on_device=True,
                   out_on_device=True)
    got, _ = G.decrypt_decode(sk[0], out.data_ptr(), count=len(bundles), on_device=True, want_blocks=False)
    found = {}
    for l in occ:
        s = (int(l) % ipb) * F
        found[int(table_idx[l])] = any((got[b, s:s + F] == mask_vals[b, s:s + F]).all() for b in range(len(bundles)))
    assert len(found) == 128 and all(found[i] == bool(in_db[i]) for i in range(128))
    assert found[0] and not found[127]                                     # an inserted item is found, a fresh one is missed
    G.close()
