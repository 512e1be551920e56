"""GPU tier of find-and-place: apsu_he_bundle_bin_counts, apsu_he_bundles_lookup and apsu_he_db_apply_entries on resident BinBundles
(k_bin_counts, k_bins_lookup behind Engine::decode_bundle; the placement rule of db_place.h).  The ground truth is the Python model
of this file and of tests/test_bundle_lookup_cpu.py: bins kept as lists, items as (start bin, field elements).  All comparisons are
exact integers; the BinBundles that apply_entries returns are held byte for byte to build_bundle of the model's final bins."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import apsu_amd
import common
import test_bundle_lookup_cpu as M
import test_gpu_bundle_update as U
from apsu_amd.engine import load_library
from oracle import ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFF
F = 5                                                     # felts_per_item of toy_json and of the shipped parameter sets used here


def make_db(rng, t, bins, per_start, starts, avoid_zero=True):
    """items (start, felts) with per_start(s) items at each start bin of `starts` -> (items, bins as lists).  Values are distinct within a
    bin, so an item assembled from parts of different items is a false positive and nothing else."""
    out = [[] for _ in range(bins)]
    items = []
    for s in starts:
        for _ in range(per_start(s)):
            f = [U.distinct(rng, t, 1, avoid=out[s + j])[0] for j in range(F)]
            items.append((s, f))
            for j in range(F):
                out[s + j].append(f[j])
    return items, out


def absent_variant(rng, t, item, bins):
    s, f = item
    f = list(f)
    j = int(rng.integers(0, F))
    f[j] = U.distinct(rng, t, 1, avoid=bins[s + j])[0]
    return (s, f)


def false_positive(a, b):
    """parts 0, 2, 4 of item a and parts 1, 3 of item b (same start bin)"""
    assert a[0] == b[0] and a[1] != b[1]
    return (a[0], [a[1][j] if j % 2 == 0 else b[1][j] for j in range(F)])


def model_present(bins, e):
    s, f = e
    return all(s + j < len(bins) and bins[s + j] is not None and f[j] in bins[s + j] for j in range(F))


def model_room(bins, e):
    s, f = e
    if any(s + j >= len(bins) or bins[s + j] is None for j in range(F)):
        return NONE
    return max(len(bins[s + j]) + 1 for j in range(F))


def check_lookup(G, gb, bins, entries):
    present, room = G.lookup([gb], entries)
    assert [bool(v) for v in present[0]] == [model_present(bins, e) for e in entries]
    assert [int(v) for v in room[0]] == [model_room(bins, e) for e in entries]
    return present[0]


def three_kinds(rng, t, items, bins, k):
    """explicit thirds: k items that are in, k with one part replaced by a value its bin does not hold, k false positives"""
    by_start = {}
    for it in items:
        by_start.setdefault(it[0], []).append(it)
    pairs = [(v[i], v[i + 1]) for v in by_start.values() for i in range(len(v) - 1)]
    assert len(pairs) >= k and len(items) >= k
    inside = [items[int(i)] for i in rng.choice(len(items), size=k, replace=False)]
    absent = [absent_variant(rng, t, it, bins) for it in inside]
    fps = [false_positive(*pairs[int(i)]) for i in rng.choice(len(pairs), size=k, replace=False)]
    # the model itself yields the three kinds
    assert all(model_present(bins, e) for e in inside)
    assert not any(model_present(bins, e) for e in absent)
    assert all(model_present(bins, e) and e not in items for e in fps)
    return inside + absent + fps


def toy_db(rng, t):
    """ragged toy bins: start bins 0, 5, .. 55 with 0 .. 6 items each, start bin 15 left empty, root 0 in bin 7"""
    items, bins = make_db(rng, t, 60, lambda s: 0 if s == 15 else 2 if s == 0 else int(rng.integers(2, 7)), range(0, 60, F))
    s, f = items[2]
    assert s == 5
    bins[7].remove(f[2])
    f[2] = 0
    bins[7].append(0)
    return items, bins


def test_counts_and_lookup_on_ragged_toy_bins():
    js = common.toy_json()
    rng = np.random.default_rng(31)
    t = U.toy_t()
    items, bins = toy_db(rng, t)
    assert bins[15] == [] and 0 in bins[7]
    G = apsu_amd.HeContext(js)
    gb = G.build_bundle(0, 0, bins)
    assert [int(v) for v in G.bin_counts(gb)] == [len(b) for b in bins] + [NONE] * 4
    entries = three_kinds(rng, t, items, bins, 8) + [items[2], (5, [items[2][1][0], items[2][1][1], 1, items[2][1][3], items[2][1][4]])]
    got = check_lookup(G, gb, bins, entries)
    assert [bool(v) for v in got[:24]] == [True] * 8 + [False] * 8 + [True] * 8 and bool(got[24]) and not bool(got[25])
    # an empty bin (the polynomial 1) holds nothing; entries may start at any bin
    check_lookup(G, gb, bins, [(15, [0] * F), (15, [1] * F), (13, items[2][1]), (55, items[-1][1]), (3, [bins[3 + j][0] for j in range(F)])])
    # a skewed batch: 200 entries at one start bin
    skew = [items[0] if k % 3 == 0 else absent_variant(rng, t, items[0], bins) for k in range(200)]
    skew = [(0, f) for _, f in skew]
    got = check_lookup(G, gb, bins, skew)
    assert 0 < sum(bool(v) for v in got) < 200
    # several BinBundles in one call, decoded one after the other
    items2, bins2 = make_db(rng, t, 60, lambda s: 3, range(0, 60, F))
    gb2 = G.build_bundle(0, 1, bins2)
    both = entries + items2[:6]
    present, room = G.lookup([gb, gb2], both)
    for row, bb in ((0, bins), (1, bins2)):
        assert [bool(v) for v in present[row]] == [model_present(bb, e) for e in both]
        assert [int(v) for v in room[row]] == [model_room(bb, e) for e in both]
    assert present[1].any() and present[0].any()
    G.close()


def test_partly_built_bundle_has_no_bins_beyond_what_it_was_given():
    js = common.toy_json()
    rng = np.random.default_rng(32)
    t = U.toy_t()
    items, bins = make_db(rng, t, 40, lambda s: 3, range(0, 40, F))
    G = apsu_amd.HeContext(js)
    gb = G.build_bundle(0, 0, bins)
    assert [int(v) for v in G.bin_counts(gb)] == [3] * 40 + [NONE] * 24
    entries = [items[0], (36, items[-1][1]), (38, [0] * F), (40, [1] * F), (55, [2] * F), (35, items[-1][1])]
    present, room = G.lookup([gb], entries)
    assert [bool(v) for v in present[0]] == [True, False, False, False, False, True]
    assert [int(v) for v in room[0]] == [4, NONE, NONE, NONE, NONE, 4]
    G.close()


def test_long_horner_chains():
    js = common.toy_json(ps_low=0, max_items=210, query_powers=(1,))
    rng = np.random.default_rng(33)
    t = U.toy_t(js)
    sizes = {0: 200, 5: 63, 10: 64, 15: 65, 20: 1, 25: 129}
    items, bins = make_db(rng, t, 60, lambda s: sizes.get(s, 2), range(0, 60, F))
    G = apsu_amd.HeContext(js)
    gb = G.build_bundle(0, 0, bins)
    assert gb.degree == 200
    assert [int(v) for v in G.bin_counts(gb)] == [len(b) for b in bins] + [NONE] * 4
    check_lookup(G, gb, bins, three_kinds(rng, t, items, bins, 30))
    G.close()


def big_db(rng, js):
    p = ref.load_params(js)
    C_ = ref.RefContext.from_params(p)
    assert p["felts_per_item"] == F
    n_bins = p["items_per_bundle"] * F
    assert (C_.n, n_bins) == (4096, 4095)
    starts = sorted(set([60, 4090, 0, 4030] + [int(v) * F for v in rng.choice(n_bins // F, size=60, replace=False)]))
    items, bins = make_db(rng, C_.t, n_bins, lambda s: int(rng.integers(2, 7)), starts)
    return C_.t, n_bins, items, bins


def big_entries(rng, t, items, bins):
    entries = three_kinds(rng, t, items, bins, 60)
    straddle = next(it for it in items if it[0] == 60)     # slots 60 .. 64: two tiles
    last = next(it for it in items if it[0] == 4090)       # ends in bin 4094, the last one; slot 4095 is unused
    entries += [straddle, last, absent_variant(rng, t, last, bins), (62, [1] * F), (4090, [0] * F)]
    return entries


def test_lookup_1M_across_tile_borders():
    rng = np.random.default_rng(34)
    js = common.param_json("1M-1024-com")
    t, n_bins, items, bins = big_db(rng, js)
    G = apsu_amd.HeContext(js)
    gb = G.build_bundle(0, 0, bins)
    counts = G.bin_counts(gb)
    assert [int(v) for v in counts[:n_bins]] == [len(b) for b in bins] and int(counts[4095]) == NONE
    entries = big_entries(rng, t, items, bins)
    got = check_lookup(G, gb, bins, entries)
    assert bool(got[180]) and bool(got[181]) and not bool(got[182])
    with pytest.raises(ValueError, match="bins_per_bundle"):
        G.lookup([gb], [(4091, [1] * F)])                  # would touch slot 4095
    with pytest.raises(ValueError, match="not reduced"):
        G.lookup([gb], [(0, [1, 2, t, 3, 4])])
    G.close()


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np, apsu_amd, common, test_gpu_bundle_lookup as T
rng = np.random.default_rng(35)
t = T.U.toy_t()
items, bins = T.toy_db(rng, t)
entries = T.three_kinds(rng, t, items, bins, 8)
G = apsu_amd.HeContext(common.toy_json())
gb = G.build_bundle(0, 0, bins)
present, room = G.lookup([gb], entries)
np.savez(sys.argv[3], row_format=G.save_bundle(gb)[:256], counts=G.bin_counts(gb), present=present, room=room)
"""


def test_lookup_after_save_load_and_on_dense_rows(tmp_path):
    js = common.toy_json()
    rng = np.random.default_rng(35)
    t = U.toy_t()
    items, bins = toy_db(rng, t)
    entries = three_kinds(rng, t, items, bins, 8)
    G = apsu_amd.HeContext(js)
    gb = G.build_bundle(0, 0, bins)
    image = G.save_bundle(gb)
    assert int(image[8 + 16 + 88 + 8 + 28:][:4].view(np.uint32)[0]) == 1, "this context keeps packed rows"
    want = check_lookup(G, gb, bins, entries)
    G2 = apsu_amd.HeContext(js)                            # knows the image only
    loaded = G2.load_bundle(image)
    assert (check_lookup(G2, loaded, bins, entries) == want).all()
    assert (G2.bin_counts(loaded) == G.bin_counts(gb)).all()
    G2.close()
    # dense 64-bit rows: APSU_HE_PACKED_ROWS is read when a context is created, so that BinBundle is built in a fresh process
    dst = str(tmp_path / "dense.npz")
    env = dict(os.environ, APSU_HE_PACKED_ROWS="0")
    subprocess.run([sys.executable, "-c", CHILD, os.path.dirname(HERE), HERE, dst], env=env, check=True, timeout=120)
    got = np.load(dst)
    assert int(got["row_format"][8 + 16 + 88 + 8 + 28:][:4].view(np.uint32)[0]) == 0, "the child kept dense rows"
    assert (got["counts"] == G.bin_counts(gb)).all()
    assert (got["present"][0] == want).all() and [int(v) for v in got["room"][0]] == [model_room(bins, e) for e in entries]
    G.close()


def poly_eval_slots(bins, x, t, n):
    """P_bin(x_slot) mod t per slot; 0 where the slot is not a bin"""
    out = np.zeros(n, dtype=object)
    for s, b in enumerate(bins):
        acc = 1
        for r in b:
            acc = acc * (int(x[s]) - r) % t
        out[s] = acc
    return out


def apply_scene(rng, t):
    """three BinBundles of bundle index 1 (every state needs its own BinBundle) and a batch that meets every status"""
    # b0: start bins 0 and 5 full (10 = max_items_per_bin - 1 items per bin), the rest ragged
    items0, bins0 = make_db(rng, t, 60, lambda s: 10 if s in (0, 5) else 2, range(0, 60, F))
    # b1: start bin 0 full too, start bin 5 at 9, the rest ragged
    items1, bins1 = make_db(rng, t, 60, lambda s: {0: 10, 5: 9}.get(s, 3), range(0, 60, F))
    # b2: one single item
    items2, bins2 = make_db(rng, t, 60, lambda s: 1 if s == 20 else 0, range(0, 60, F))
    at = lambda items, s: [it for it in items if it[0] == s]
    new = lambda s: (s, U.distinct(rng, t, F, avoid=[v for b in (bins0, bins1, bins2) for v in b[s] + b[s + 1] + b[s + 2] + b[s + 3] + b[s + 4]]))
    e_over, e_fill, e_next = new(0), new(5), new(5)
    inserts = [new(10),                                    # INSERTED into b1: the newest that is not EMPTY
               at(items0, 30)[0],                          # DUPLICATE: b0 holds it
               false_positive(*at(items1, 35)[:2]),        # DUPLICATE: the false positive
               new(20),                                    # b2 is EMPTY by then and takes nothing: b1
               e_fill,                                     # takes b1's start bin 5 from 9 to 10 ...
               e_next,                                     # ... so this one finds no room in b1, none in b0: a new BinBundle
               e_over,                                     # start bin 0 is full in b1 and b0; the new BinBundle is the newest by now
               e_over]                                     # DUPLICATE of an entry placed by this call
    removes = [items2[0],                                  # empties b2
               at(items1, 40)[1],                          # REMOVED from b1
               absent_variant(rng, t, at(items0, 45)[0], bins0),   # NOT_FOUND
               at(items1, 10)[0]]
    return [bins0, bins1, bins2], inserts, removes


def test_apply_entries_every_status_and_state():
    js = common.toy_json()
    rng = np.random.default_rng(36)
    t = U.toy_t()
    model, inserts, removes = apply_scene(rng, t)
    want = M.model_place(model, inserts, removes, F, 60, 11)
    final = want.pop("final")
    assert want["ins_status"] == [M.INSERTED, M.DUPLICATE, M.DUPLICATE, M.INSERTED, M.INSERTED, M.INSERTED, M.INSERTED, M.DUPLICATE]
    assert want["ins_target"] == [1, 0, 1, 1, 1, 3, 3, 3]
    assert want["rem_status"] == [M.REMOVED, M.REMOVED, M.NOT_FOUND, M.REMOVED] and want["rem_target"] == [2, 1, NONE, 1]
    assert want["state"] == [M.UNCHANGED, M.REPLACED, M.EMPTY] and want["n_new"] == 1

    S = common.make_scenario(js, {1: []})
    G = apsu_amd.HeContext(js)
    old = [G.build_bundle(1, c, b) for c, b in zip((0, 2, 5), model)]
    before = [G.save_bundle(b).tobytes() for b in old]
    res = G.apply_entries(old, inserts=inserts, removes=removes)
    assert [int(v) for v in res.state] == want["state"]
    assert [int(v) for v in res.ins_status] == want["ins_status"] and [int(v) for v in res.ins_target] == want["ins_target"]
    assert [int(v) for v in res.rem_status] == want["rem_status"] and [int(v) for v in res.rem_target] == want["rem_target"]
    assert [b is not None for b in res.bundles] == [False, True, False] and len(res.appended) == 1
    assert [G.save_bundle(b).tobytes() for b in old] == before            # the given BinBundles are only read
    up, app = res.bundles[1], res.appended[0]
    assert (up.bundle_idx, up.cache_idx) == (1, 2) and (app.bundle_idx, app.cache_idx) == (1, 6)
    assert all(len(b) <= 10 for bb in final for b in bb)
    assert G.save_bundle(up).tobytes() == G.save_bundle(G.build_bundle(1, 2, final[1])).tobytes()
    assert G.save_bundle(app).tobytes() == G.save_bundle(G.build_bundle(1, 6, final[3])).tobytes()
    assert not any(final[2][s] for s in range(60))
    # the database after the call answers for itself
    db = [old[0], up, app]
    present, _ = G.lookup(db, inserts + removes)
    assert present[:, :len(inserts)].any(axis=0).all()
    assert [bool(v) for v in present[:, len(inserts):].any(axis=0)] == [False, False, False, False]
    # one query on the result: P(x) + mask for the model's bins
    rk = G.upload_relin_keys(S.rk)
    pw = G.compute_powers([1], [[S.src[1][e] for e in S.sources]], rk)
    mask_vals = ref.fill_uniform(9, S.C.t, S.C.n)
    masks = [S.C.encode(mask_vals)] * 3
    out = G.eval_bundles(db, pw, rk, masks)
    for i, bb in enumerate((final[0], final[1], final[3])):
        got = S.C.decode(S.C.decrypt(S.sk, np.ascontiguousarray(out[i]), 0)[0]).astype(object)
        exp = (poly_eval_slots(bb, S.x[1], t, S.C.n) + mask_vals.astype(object)) % t
        exp[60:] = mask_vals[60:]
        assert (got == exp).all(), i
    G.close()


def test_apply_entries_from_nothing_and_without_changes():
    js = common.toy_json()
    rng = np.random.default_rng(37)
    t = U.toy_t()
    items, bins = make_db(rng, t, 60, lambda s: 2, range(0, 60, F))
    G = apsu_amd.HeContext(js)
    res = G.apply_entries([], inserts=items, bundle_idx=1)
    assert len(res.appended) == 1 and (res.appended[0].bundle_idx, res.appended[0].cache_idx) == (1, 0)
    assert G.save_bundle(res.appended[0]).tobytes() == G.save_bundle(G.build_bundle(1, 0, bins)).tobytes()
    again = G.apply_entries(res.appended, inserts=items[:5], removes=[absent_variant(rng, t, items[0], bins)])
    assert [int(v) for v in again.state] == [M.UNCHANGED] and again.bundles == [None] and again.appended == []
    assert [int(v) for v in again.ins_status] == [M.DUPLICATE] * 5 and [int(v) for v in again.rem_status] == [M.NOT_FOUND]
    G.close()


def raw_apply(G, bundle_idx, bundles, ins, rem):
    """the C call itself, its outputs pre-set: -> (status, last error, replaced handles, appended handles, n_appended)"""
    L = load_library()
    fi = np.ascontiguousarray([f for _, f in ins], dtype=np.uint64).reshape(-1, F)
    si = np.ascontiguousarray([s for s, _ in ins], dtype=np.uint32)
    fr = np.ascontiguousarray([f for _, f in rem], dtype=np.uint64).reshape(-1, F)
    sr = np.ascontiguousarray([s for s, _ in rem], dtype=np.uint32)
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    u32 = lambda a: C.c_void_p(a.ctypes.data)
    nb = len(bundles)
    hs = (C.c_void_p * max(nb, 1))(*[b.h for b in bundles])
    state = np.full(max(nb, 1), 77, dtype=np.uint32)
    replaced = (C.c_void_p * max(nb, 1))()
    appended = (C.c_void_p * max(len(si), 1))()
    n_app = C.c_uint32(77)
    rc = L.apsu_he_db_apply_entries(G.h, C.c_uint32(bundle_idx), hs, nb, u64(fi), u32(si), C.c_size_t(len(si)), u64(fr), u32(sr), C.c_size_t(len(sr)),
                                    u32(state), replaced, appended, C.byref(n_app), None, None, None, None)
    return rc, L.apsu_he_last_error().decode(), [h for h in replaced], [h for h in appended], n_app.value


def test_apply_entries_refusals_leave_no_handle():
    js = common.toy_json()
    rng = np.random.default_rng(38)
    t = U.toy_t()
    items, bins = make_db(rng, t, 60, lambda s: 3, range(0, 60, F))
    G = apsu_amd.HeContext(js)
    b0, b1, other = G.build_bundle(0, 0, bins), G.build_bundle(0, 1, bins), G.build_bundle(1, 2, bins)
    fresh = (0, U.distinct(rng, t, F, avoid=[v for s in range(F) for v in bins[s]]))
    a, b = items[0], items[1]
    shares_part_0 = (0, [a[1][0]] + b[1][1:])              # present (a false positive); bin 0 holds a's part once
    cases = [([b0, b1], [fresh], [fresh], "removal list too"),
             ([b0, b1], [], [a, b, a], "twice"),
             ([b0, b1], [(0, [1, 2, 3, 4, t])], [], "not reduced"),
             ([b0, b1], [fresh], [(5, [t + 1, 2, 3, 4, 5])], "not reduced"),
             ([b0, b1], [(56, [1, 2, 3, 4, 5])], [], "bins_per_bundle"),
             ([b0, other], [fresh], [], "one bundle index"),
             ([b1, b0], [fresh], [], "cache order"),
             ([b0, b1], [fresh], [a, shares_part_0], "is not a root")]           # found late, by the update's division
    for bundles, ins, rem, text in cases:
        rc, err, replaced, appended, n_app = raw_apply(G, 0, bundles, ins, rem)
        assert rc == -1 and text in err, (rc, err)
        assert not any(replaced) and not any(appended) and n_app == 77
        with pytest.raises(ValueError, match=text):
            G.apply_entries(bundles, inserts=ins, removes=rem, bundle_idx=0)
    # the context and the BinBundles are as they were
    rc, err, replaced, appended, n_app = raw_apply(G, 0, [b0, b1], [fresh], [a])
    assert rc == 0 and n_app == 0 and replaced[0] and replaced[1]       # a leaves b0 (the first holder), fresh goes to b1 (the newest)
    for h in replaced:
        load_library().apsu_he_bundle_free(C.c_void_p(h))
    G.close()
