"""GPU tier: cuckoo hashing on the device (kernels_cuckoo.hip: k_cuckoo_locations, k_cuckoo_insert, k_query_values) against the
independent model tests/cuckoo_model.py, bit for bit, and the two parties end to end: items inserted into a resident database through
insert_items are found by a query built through cuckoo_table and query_values, and only they."""
import json

import numpy as np
import pytest

import apsu_amd
import common
import cuckoo_cases
import cuckoo_model as M
from apsu_amd import seal, wire

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED = bytes((13 * i + 5) & 0xFF for i in range(64))
LDS_SLOTS = (65536 - 64) // 8           # what k_cuckoo_insert's LDS form holds (cuckoo.h: CUCKOO_LDS_SLOTS)


def toy_with(H, table_mult=3):
    js = json.loads(common.toy_json(table_mult=table_mult))
    js["table_params"]["hash_func_count"] = H
    return json.dumps(js)


@pytest.fixture(scope="module")
def toy():
    G = apsu_amd.HeContext(common.toy_json())
    yield G
    G.close()


def random_items(count, seed):
    return np.random.default_rng(seed).integers(0, 256, (count, 16), dtype=np.uint8)


def model_locations(items, H, T):
    return M.locations([bytes(it) for it in items], H, T)


# ---- locations
@pytest.mark.parametrize("H", [1, 3, 8])
def test_item_locations_equal_the_model(H):
    """H = 1, 3, 8: one, one and two staging groups of the tables; T = 36, not a power of two; host and device pointers"""
    G = apsu_amd.HeContext(toy_with(H))
    T = G.table_size
    assert T == 36 and G.hash_func_count == H
    items = random_items(1000, 100 + H)
    want = np.array(model_locations(items, H, T), dtype=np.uint32).reshape(-1, H)
    for count in (0, 1, 63, 64, 65, 1000):
        got = G.item_locations(items[:count])
        assert got.shape == (count, H) and (got == want[:count]).all(), count
    d_items = torch.from_numpy(items).cuda()
    d_locs = torch.full((1000 * H + 1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                                               # (the engine's stream does not wait for torch's)
    assert G.item_locations(d_items.data_ptr(), count=1000, locs=d_locs.data_ptr()) is None
    back = d_locs.cpu().numpy().view(np.uint32)
    assert (back[:-1].reshape(1000, H) == want).all() and back[-1] == 0xFFFFFFFF      # nothing behind count * H is written
    # items at an address that is not a multiple of 16 (the kernel loads 16 bytes at once: the engine moves them)
    d_odd = torch.zeros(16 * 65 + 4, dtype=torch.uint8, device="cuda")
    d_odd[4:] = d_items[:65].reshape(-1)
    torch.cuda.synchronize()
    G.item_locations(d_odd.data_ptr() + 4, count=65, locs=d_locs.data_ptr())
    assert (d_locs.cpu().numpy().view(np.uint32)[:65 * H].reshape(65, H) == want[:65]).all()
    G.close()


@pytest.mark.parametrize("H,T", [(3, 1), (8, 1 << 30), (5, 6552), (1, 409)])
def test_location_kernel_alone_at_the_table_sizes_no_toy_context_has(toy, H, T):
    """T = 1 (every location 0), the largest table, H = 5 (a full staging group and a partial one); more than one workgroup"""
    items = random_items(2500, 7 * H + T % 1000)
    items[0], items[1] = 0, 255
    got = toy.debug_item_locations(items, H, T)
    assert (got == np.array(model_locations(items, H, T), dtype=np.uint32)).all()
    assert (got < T).all()


def test_location_kernel_with_persistent_workgroups():
    """more items than the grid has lanes: every workgroup walks its stride (1.2 M items: 2 workgroups per compute unit hold 0.5 M)"""
    G = apsu_amd.HeContext(common.param_json("16M-4096"))
    items = random_items(1_200_000, 9)
    got = G.item_locations(items)
    pick = np.random.default_rng(1).choice(len(items), 600, replace=False)
    pick = np.concatenate([pick, [0, len(items) - 1, 1024 * 512 - 1, 1024 * 512]])
    assert (got[pick] == np.array(model_locations(items[pick], 3, 6552), dtype=np.uint32)).all()
    assert (got < 6552).all()
    G.close()


# ---- the table rule on given locations
def held_against_model(G, case, form):
    name, items, locs, H, T, max_rounds, succeeds = case
    want = M.insert(list(items), locs.tolist(), H, T, max_rounds)
    assert want.ok == succeeds, name
    if not succeeds:
        with pytest.raises(apsu_amd.ApsuHeError) as e:
            G.debug_cuckoo_insert(items, locs, T, max_rounds, form)
        msg = str(e.value)
        assert "status -3" in msg and "item %d " % want.unplaced in msg and "%d rounds" % want.rounds in msg and "%.3f" % want.fill in msg, msg
        return
    table_idx, item_loc, rounds = G.debug_cuckoo_insert(items, locs, T, max_rounds, form)
    assert rounds == want.rounds, name
    assert table_idx.tolist() == want.table_idx and item_loc.tolist() == want.item_loc, name


@pytest.mark.parametrize("form", [1, 2])
def test_collision_cases_equal_the_model_in_both_forms(toy, form):
    for case in cuckoo_cases.collision_cases():
        held_against_model(toy, case, form)


@pytest.mark.parametrize("form", [0, 1, 2])
def test_more_items_than_lanes(toy, form):
    """1025 items: lane 0 has two, the others one; and 3000 items with repeats in 4500 slots: up to three items per lane"""
    held_against_model(toy, cuckoo_cases.random_case(1025, 2048, 3, 1), form)
    held_against_model(toy, cuckoo_cases.random_case(3000, 4500, 3, 2, duplicates=40), form)


def test_largest_shipped_pair_and_the_lds_limit(toy):
    """11 041 items in 16 380 slots: device memory takes it, LDS refuses it; the engine's choice is device memory there and LDS at the
    largest table that fits"""
    case = cuckoo_cases.random_case(11041, 16380, 3, 3)
    held_against_model(toy, case, 2)
    held_against_model(toy, case, 0)
    with pytest.raises(apsu_amd.ApsuHeError) as e:
        toy.debug_cuckoo_insert(case[1], case[2], 16380, 500, 1)
    assert "status -2" in str(e.value) and "LDS" in str(e.value)
    edge = cuckoo_cases.random_case(5000, LDS_SLOTS, 3, 4)
    for form in (0, 1, 2):
        held_against_model(toy, edge, form)
    with pytest.raises(apsu_amd.ApsuHeError):
        toy.debug_cuckoo_insert(edge[1][:4], edge[2][:4], LDS_SLOTS + 1, 500, 1)
    held_against_model(toy, cuckoo_cases.random_case(4, LDS_SLOTS + 1, 3, 5), 0)


def test_failure_returns_its_status_and_the_context_goes_on(toy):
    case = [c for c in cuckoo_cases.collision_cases() if c[0] == "three items on two locations"][0]
    for form in (1, 2):
        held_against_model(toy, case, form)
    ok = [c for c in cuckoo_cases.collision_cases() if c[0] == "eviction chain"][0]
    held_against_model(toy, ok, 0)


def test_insert_refusals(toy):
    items = random_items(2, 1)
    locs = np.array([[0, 1], [1, 0]], dtype=np.uint32)
    for bad_rounds in (0, (1 << 32) + 1):
        with pytest.raises(ValueError):
            toy.debug_cuckoo_insert(items, locs, 2, bad_rounds, 0)
    with pytest.raises(ValueError):
        toy.debug_cuckoo_insert(items, locs, 1, 500, 0)                   # a location outside the table
    with pytest.raises(ValueError):
        toy.debug_cuckoo_insert(items, locs, 2, 500, 3)                   # no such form
    with pytest.raises(ValueError):
        toy.cuckoo_table(items, max_rounds=0)
    assert toy.debug_cuckoo_insert(items, locs, 2, 1 << 32, 0)[2] == 1
    raw = apsu_amd.HeContext(n=toy.n, coeff_modulus=toy.q, plain_modulus=toy.t)
    with pytest.raises(apsu_amd.ApsuHeError):                              # a context without PSUParams has no table
        raw.item_locations(items)
    import ctypes as C
    out = np.zeros((2, 3), dtype=np.uint32)
    rc = apsu_amd.load_library().apsu_he_item_locations(raw.h, C.c_void_p(items.ctypes.data), C.c_size_t(2), 0, C.c_void_p(out.ctypes.data), 0)
    assert rc == -2                                                        # APSU_HE_LOGIC_ERROR, as the other N1 calls refuse it
    raw.close()


# ---- the public calls on real locations
@pytest.mark.parametrize("name,count", [("toy", 12), ("256K-512", 512), ("16M-4096", 4096), ("16M-11041", 11041)])
def test_cuckoo_table_equals_the_model(name, count):
    """LDS tables (toy, 819, 6552 slots) and the one in device memory (16 380); repeated items among them"""
    G = apsu_amd.HeContext(common.toy_json() if name == "toy" else common.param_json(name))
    T, H = G.table_size, G.hash_func_count
    items = random_items(count, count)
    items[count // 2] = items[3]
    items[count - 1] = items[3]
    locs = G.item_locations(items)
    if count <= 512:
        assert locs.tolist() == model_locations(items, H, T)
    want = M.insert(list(items), locs.tolist(), H, T)
    assert want.ok
    table_idx, item_loc, rounds = G.cuckoo_table(items)
    assert rounds == want.rounds and table_idx.tolist() == want.table_idx and item_loc.tolist() == want.item_loc
    M.check_invariants(list(items), locs.tolist(), want)
    assert item_loc[count // 2] == M.NONE and item_loc[count - 1] == M.NONE and item_loc[3] != M.NONE
    e_idx, e_loc, e_rounds = G.cuckoo_table(items[:0])
    assert (e_idx == M.NONE).all() and len(e_loc) == 0 and e_rounds == 0
    G.close()


def test_bucket_items_equals_the_model(toy):
    items = random_items(200, 5)
    items[17] = items[4]                                                   # (a repeated item is listed twice: the database side does not dedupe)
    offsets, order = toy.bucket_items(items)
    want_off, want_order = M.bucket(model_locations(items, 3, toy.table_size), toy.table_size)
    assert offsets.tolist() == want_off and order.tolist() == want_order
    off0, order0 = toy.bucket_items(items[:0])
    assert (off0 == 0).all() and len(order0) == 0


@pytest.mark.parametrize("name", ["256K-512", "1M-256", "toy"])
def test_query_values_is_algebraize_plus_the_layout(name):
    """T = 819, F = 5 and T = 585, F = 7 (n = 4096: 1 and 1 positions of padding ... 4095 and 4095 used), the toy with two bundle indices"""
    G = apsu_amd.HeContext(common.toy_json() if name == "toy" else common.param_json(name))
    T, F, n, ipb = G.table_size, G.felts_per_item, G.n, int(G.info.items_per_bundle)
    table_items = random_items(T, T)
    table_items[1] = 0
    table_items[2] = 255
    felts = G.algebraize_items(table_items)
    want = np.zeros((G.bundle_idx_count, n), dtype=np.uint64)
    for b in range(G.bundle_idx_count):
        want[b, :ipb * F] = felts[b * ipb:(b + 1) * ipb].reshape(-1)
    assert ipb * F < n or name == "toy"                                    # there is padding to check
    got = G.query_values(table_items)
    assert (got == want).all() and (got < G.t).all()
    d_items = torch.from_numpy(table_items).cuda()
    d_vals = torch.full((G.bundle_idx_count * n + 1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert G.query_values(d_items.data_ptr(), values=d_vals.data_ptr()) is None
    back = d_vals.cpu().numpy().view(np.uint64)
    assert (back[:-1].reshape(want.shape) == want).all() and back[-1] == 0xFFFFFFFFFFFFFFFF
    G.close()


# ---- both parties
def model_felts(item, F, bpf):
    v = int.from_bytes(bytes(item), "little") & ((1 << (F * bpf)) - 1)
    return [(v >> (j * bpf)) & ((1 << bpf) - 1) for j in range(F)]


def test_both_sides_agree_end_to_end():
    """256K-512: 300 items into an empty resident database through insert_items (identity OPRF); 128 query items, 64 of them in the
    database, through cuckoo_table -> query_values -> query_create -> compute_powers -> eval_bundles -> decrypt_decode.  An occupied slot
    decrypts to the mask in all felts of its item, in some BinBundle, iff the item is in the database.  The protocol (the reference's too)
    reports a false positive when every felt of a query item lies in its bin, each from another database item; the seed is one where the
    model shows none, which the test asserts before it looks at the GPU."""
    js = common.param_json("256K-512")
    G = apsu_amd.HeContext(js)
    T, H, F, n, ipb, t = G.table_size, G.hash_func_count, G.felts_per_item, G.n, int(G.info.items_per_bundle), G.t
    bpf = t.bit_length() - 1
    assert (T, H, F, n, G.bundle_idx_count) == (819, 3, 5, 4096, 1)
    rng = np.random.default_rng(0x32353651)
    db = rng.integers(0, 256, (300, 16), dtype=np.uint8)
    query = np.concatenate([db[rng.choice(300, 64, replace=False)], rng.integers(0, 256, (64, 16), dtype=np.uint8)])
    in_db = np.arange(128) < 64
    # the model's database: per bin the felts the bucketed items put there
    db_locs = model_locations(db, H, T)
    want_off, want_order = M.bucket(db_locs, T)
    bins = [[] for _ in range(ipb * F)]
    for l in range(T):
        for i in want_order[want_off[l]:want_off[l + 1]]:
            for j, f in enumerate(model_felts(db[i], F, bpf)):
                bins[(l % ipb) * F + j].append(f)
    q_locs = model_locations(query, H, T)
    q_table = M.insert(list(query), q_locs, H, T)
    assert q_table.ok
    for i in range(128):                                                   # the precondition: no cross-item false positive in the model
        s = (q_table.item_loc[i] % ipb) * F
        hit = all(f in bins[s + j] for j, f in enumerate(model_felts(query[i], F, bpf)))
        assert hit == bool(in_db[i])
    # the database side
    res = G.insert_items({}, db)
    assert sorted(res) == [0] and (res[0].ins_status == apsu_amd.engine.ENTRY_INSERTED).all()
    bundles = res[0].appended
    assert len(bundles) >= 1
    offsets, order = G.bucket_items(db)
    assert offsets.tolist() == want_off and order.tolist() == want_order
    (lo, hi, start), = G.bucket_entries(offsets)
    assert (lo, hi) == (0, len(order)) and start.tolist() == [(l % ipb) * F for l in range(T) for _ in range(want_off[l + 1] - want_off[l])]
    present, _ = G.lookup(bundles, (G.algebraize_items(db[order]), start))
    assert present.any(axis=0).all()
    sc = seal.SealContext(js)
    held = [[] for _ in range(ipb * F)]
    for b in bundles:
        got_bins = wire.parse_bin_bundle(seal.export_saved_bundle(G, sc, b))["item_bins"]
        for s, x in enumerate(got_bins):
            held[s] += [int(v) for v in x]
    assert [sorted(x) for x in held] == [sorted(x) for x in bins]
    # the querier's side
    table_idx, item_loc, rounds = G.cuckoo_table(query)
    assert table_idx.tolist() == q_table.table_idx and item_loc.tolist() == q_table.item_loc and rounds == q_table.rounds
    table_items = np.zeros((T, 16), dtype=np.uint8)
    occ = np.nonzero(table_idx != M.NONE)[0]
    table_items[occ] = query[table_idx[occ]]
    S, L = G.source_power_count, G.first_chain_idx + 1
    d_vals = torch.zeros(n, dtype=torch.int64, device="cuda")
    cts = torch.zeros((S, 2, L, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()                                               # (the engine's stream does not wait for torch's)
    G.query_values(table_items, values=d_vals.data_ptr())
    sk = G.keygen(SEED)
    _, _, rk = G.relin_keygen(sk, SEED, want_host=False)
    G.query_create(sk, [0], d_vals.data_ptr(), cts.data_ptr(), seed=SEED, values_on_device=True)
    pw = G.compute_powers([0], [[cts.data_ptr() + s * 2 * L * n * 8 for s in range(S)]], rk, on_device=True)
    mbuf = torch.empty(len(bundles) * n, dtype=torch.int64, device="cuda")
    mask_vals, _ = G.mask_generate(77, len(bundles), mbuf.data_ptr(), want_blocks=False)
    out = torch.empty((len(bundles), 2, n), dtype=torch.int64, device="cuda")
    G.eval_bundles(bundles, pw, rk, [mbuf.data_ptr() + i * n * 8 for i in range(len(bundles))], out=out.data_ptr(), masks_on_device=True,
                   out_on_device=True)
    got, _ = G.decrypt_decode(sk[0], out.data_ptr(), count=len(bundles), on_device=True, want_blocks=False)
    for l in occ:
        i = int(table_idx[l])
        s = (int(l) % ipb) * F
        found = any((got[b, s:s + F] == mask_vals[b, s:s + F]).all() for b in range(len(bundles)))
        assert found == bool(in_db[i]), (int(l), i)
    assert len(occ) == 128
    G.close()
