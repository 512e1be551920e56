"""GPU tier: apsu_he_bundle_export_saved / apsu_he_db_export_saved -- a resident database written in the reference's saved format
(apsu_amd/csrc/wire.h: build_bin_bundle; bin_rows.h / kernels_roots.hip: k_bins_rows; Engine::export_saved).  The contract: for every
flag setting upload_saved_bundle(export(b)) has the save_bundle image of b, bit for bit -- for a BinBundle built from bins, updated,
merged or loaded from an image -- the item bins are the sorted multisets, row s of felt_matching_polyns is prod (x - r) mod t, and
each plaintext is in the form the BatchedPlaintextPolyn ctor keeps it in.  Everything is exact."""
import json
import os

import numpy as np
import pytest

import apsu_amd
import common
import test_gpu_bundle_update as U
from apsu_amd import seal, wire
from test_gpu_bundle_roots import toy_bins

pytestmark = pytest.mark.gpu

FULL, STRIPPED, NO_CACHE = dict(), dict(stripped=True), dict(cache=False)


def matching(bins, t):
    out = []
    for b in bins:
        p = [1]
        for r in b:
            q = [0] * (len(p) + 1)
            for i, c in enumerate(p):
                q[i + 1] = (q[i + 1] + c) % t
                q[i] = (q[i] - c * int(r)) % t
            p = q
        out.append(p)
    return out


def pt_level(js):
    """the level bundle_layout names for the NTT-form plaintexts (bin_bundle.cpp:385-389): min(first_chain_idx, ps_low_degree ? 2 : 1)"""
    p = json.loads(js)
    K = len(p["seal_params"]["coeff_modulus_bits"])
    return min(max(K - 2, 0), 2 if p["query_params"]["ps_low_degree"] else 1)


def check_export(G, sc, js, b, B, cache_idx, compr=0, settings=(FULL, STRIPPED, NO_CACHE)):
    """B: the bins_per_bundle bins of b as lists.  Every setting reloads image-identical; the full export's fields are what they must be"""
    p = json.loads(js)
    n, t, ps = G.n, U.toy_t(js), p["query_params"]["ps_low_degree"]
    image = G.save_bundle(b).tobytes()
    for kw in settings:
        buf = seal.export_saved_bundle(G, sc, b, compr=compr, **kw)
        back, used = seal.upload_saved_bundle(G, sc, buf + b"next", cache_idx)
        assert used == len(buf)
        assert G.save_bundle(back).tobytes() == image, "reload differs from the BinBundle: %r" % (kw,)
        got = wire.parse_bin_bundle(buf)
        assert got["mod"] == t and got["stripped"] == bool(kw.get("stripped")) and got["has_cache"] == kw.get("cache", True)
        assert got["label_bins"] == 0
        if kw.get("stripped"):
            assert got["item_bins"] == [] and got["matching_polyns"] == [] and len(got["coeffs"]) == b.degree + 1
            continue
        assert got["item_bins"] == [sorted(int(v) for v in x) for x in B]
        if not kw.get("cache", True):
            assert got["coeffs"] == [] and got["matching_polyns"] == []
            continue
        assert got["matching_polyns"] == matching(got["item_bins"], t)
        assert [len(r) for r in got["matching_polyns"]] == [len(x) + 1 for x in B]
        assert len(got["coeffs"]) == b.degree + 1 == max(len(r) for r in got["matching_polyns"])
        lvl = pt_level(js)
        for d, blob in enumerate(got["coeffs"]):
            pt = sc.pt_load(blob)
            stored, kind = G.bundle_coeff(b, d)
            if d == 0 or (ps and d % (ps + 1) == 0):                   # coefficient form mod t, n coefficients, zero parms_id
                assert pt["chain_idx"] == -1 and len(pt["data"]) == n and int(pt["data"].max()) < t and kind in (0, 2)
                if d == 0:
                    assert (pt["data"] == stored).all()
            else:                                                      # the stored rows, dense, at the layout's level
                assert pt["chain_idx"] == lvl and kind == 1 and (pt["data"].reshape(lvl + 1, n) == stored).all()
    assert G.save_bundle(b).tobytes() == image                         # the BinBundle is only read


@pytest.fixture(scope="module")
def toy():
    js = common.toy_json()
    G, sc = apsu_amd.HeContext(js), seal.SealContext(js)
    yield js, G, sc, U.toy_t(js)
    G.close()
    sc.close()


def test_toy_ring_full_stripped_and_no_cache(toy):
    js, G, sc, t = toy
    B = toy_bins(t)
    b = G.build_bundle(1, 3, B)
    assert b.degree == 10
    check_export(G, sc, js, b, B, 3)
    got = wire.parse_bin_bundle(seal.export_saved_bundle(G, sc, b))
    assert got["bundle_idx"] == 1 and len(got["coeffs"]) == 11 and got["matching_polyns"][0] == [1] and got["item_bins"][4] == [0, 0, 17, 17, 99]
    assert [d for d, c in enumerate(got["coeffs"]) if sc.pt_load(c)["chain_idx"] == -1] == [0, 4, 8]
    ms = seal.export_saved_times(G)
    assert ms["decode_counts"] > 0 and ms["bins_rows"] > 0 and ms["serialise"] > 0


def two_toy_bundles(G, t):
    """toy_bins (degree 10) and 60 bins with counts 0 .. 4 that merge with it: no summed count reaches max_items_per_bin = 11"""
    B = toy_bins(t)
    rng = np.random.default_rng(17)
    B2 = [U.distinct(rng, t, min(4, 10 - len(x))) for x in B]
    assert sorted({len(x) for x in B2}) == [0, 1, 2, 3, 4]
    return G.build_bundle(0, 0, B), G.build_bundle(0, 1, B2)


def resident_calls(G, sc, a, b, x):
    """the staged calls, each the context's first of its kind -> (their results as bytes and lists, arena growths of the first export)"""
    grown = G.debug_counters()["arena_grow"]
    out = [seal.export_saved_bundle(G, sc, a)]
    grown = G.debug_counters()["arena_grow"] - grown
    out.append(seal.export_saved_bundle(G, sc, a, cache=False))
    out.append([None if v is None else v.tolist() for v in G.bins(a)])
    out.append(G.save_bundle(G.merge_bundles([a, b])).tobytes())
    res, is_bin = G.eval_plain([a, b], x, want_is_bin=True)
    return out + [res.tobytes(), is_bin.tobytes()], grown


def test_staged_calls_under_arena_retry(monkeypatch):
    """every call that runs bundle_bins' stages or the shared prologue inside its arena body gives the same bytes when the body runs
    twice: a context without a workspace grows it on the way, the overflow comes wherever the call first needs more"""
    js = common.toy_json()
    t = U.toy_t(js)
    sc = seal.SealContext(js)
    x = np.random.default_rng(18).integers(0, t, (2, 64), dtype=np.uint64)
    G0 = apsu_amd.HeContext(js)
    want, _ = resident_calls(G0, sc, *two_toy_bundles(G0, t), x)
    G0.close()
    monkeypatch.setenv("APSU_HE_ARENA_BYTES", "0")                     # (read when a context is created)
    G = apsu_amd.HeContext(js)
    got, grown = resident_calls(G, sc, *two_toy_bundles(G, t), x)
    assert grown > 0, "the first export's body did not run twice"
    assert got == want
    G.close()
    sc.close()


def test_each_clock_is_its_own(toy):
    js, G, sc, t = toy
    a, b = two_toy_bundles(G, t)
    x = np.random.default_rng(19).integers(0, t, (2, G.n), dtype=np.uint64)
    G.bins(a)
    bins_ms = G.bins_times()
    assert all(v > 0 for v in bins_ms)
    seal.export_saved_bundle(G, sc, a)
    ms = seal.export_saved_times(G)
    assert all(ms[k] > 0 for k in ("decode_counts", "bundle_bins", "bins_rows", "copies", "serialise"))
    entry = (1, [toy_bins(t)[1 + j][0] for j in range(5)])
    assert G.lookup([a], [entry])[0][0][0]
    assert all(v > 0 for v in G.lookup_times())
    assert G.bins_times() == bins_ms                                   # the export's bins and the lookup left bundle_bins' clock alone
    G.eval_plain([a, b], x)
    eval_ms = G.eval_plain_times()
    assert all(v > 0 for v in eval_ms)
    assert G.self_test([a, b]).mismatches == 0
    assert all(v > 0 for v in G.self_test_times())
    assert G.eval_plain_times() == eval_ms                             # the self-test's plaintext answer has its own copy
    assert G.bins_times() == bins_ms


def test_toy_ring_after_update_merge_and_image_round_trip(toy):
    js, G, sc, t = toy
    rng = np.random.default_rng(7)
    B = [U.distinct(rng, t, s % 5) for s in range(60)]
    b = G.build_bundle(0, 0, B)
    # 3 inserts, 2 removes
    ins, rem = [[] for _ in range(60)], [[] for _ in range(60)]
    ins[0], ins[7], ins[59] = [12345], [t - 1], [1]
    rem[3], rem[9] = [B[3][0]], [B[9][1]]
    u = G.update_bundle(b, ins, rem)
    Bu = [sorted([v for v in B[s] if v not in rem[s]] + ins[s]) for s in range(60)]
    check_export(G, sc, js, u, Bu, 0)
    # merge of two
    B2 = [U.distinct(rng, t, (s * 3) % 4) for s in range(60)]
    m = G.merge_bundles([b, G.build_bundle(0, 1, B2)])
    check_export(G, sc, js, m, [sorted(B[s] + B2[s]) for s in range(60)], 0)
    # an image round trip
    check_export(G, sc, js, G.load_bundle(G.save_bundle(u)), Bu, 0)


def test_refusals(toy):
    js, G, sc, t = toy
    # a BinBundle that was not built from bins: its polynomials do not split
    r = G.random_bundle(1, 0, 9, 5)
    image = G.save_bundle(r).tobytes()
    buf = seal.export_saved_bundle(G, sc, r, stripped=True)
    back, _ = seal.upload_saved_bundle(G, sc, buf, 0)
    assert G.save_bundle(back).tobytes() == image
    with pytest.raises(ValueError, match=r"bin \d+"):
        seal.export_saved_bundle(G, sc, r)
    assert G.save_bundle(r).tobytes() == image
    # one bin of max_items_per_bin items: build_bundle takes it, BinBundle::load's cache check would not
    rng = np.random.default_rng(9)
    B = [U.distinct(rng, t, s % 4) for s in range(60)]
    B[37] = U.distinct(rng, t, 11)
    full = G.build_bundle(0, 0, B)
    assert full.degree == 11
    for kw in (FULL, NO_CACHE):
        with pytest.raises(ValueError, match="bin 37"):
            seal.export_saved_bundle(G, sc, full, **kw)
    # plaintexts above the longest bin: BinBundle::load wants as many as the longest matching polynomial has coefficients
    short = G.build_bundle(0, 0, B[:37] + [[]] * 23)
    assert short.degree == 3
    got = wire.parse_bin_bundle(seal.export_saved_bundle(G, sc, short))
    extra = sc.pt_save(pt_level(js), np.zeros((pt_level(js) + 1) * G.n, dtype=np.uint64))
    flat = sc.pt_save(-1, np.zeros(G.n, dtype=np.uint64))             # d = 4 = ps_low_degree + 1 stays in coefficient form
    tall, _ = seal.upload_saved_bundle(G, sc, wire.build_bin_bundle(0, t, got["item_bins"], got["matching_polyns"], got["coeffs"] + [flat, extra]), 0)
    assert tall.degree == 5
    with pytest.raises(ValueError, match="degree 5 but its longest bin holds 3"):
        seal.export_saved_bundle(G, sc, tall)
    back, _ = seal.upload_saved_bundle(G, sc, seal.export_saved_bundle(G, sc, tall, stripped=True), 0)
    assert G.save_bundle(back).tobytes() == G.save_bundle(tall).tobytes()
    with pytest.raises(ValueError, match="STRIPPED and NO_CACHE"):
        seal.export_saved_bundle(G, sc, G.build_bundle(0, 0, B[:37]), stripped=True, cache=False)
    with pytest.raises(ValueError, match="compr_mode"):
        seal.export_saved_bundle(G, sc, r, stripped=True, compr=1)


def test_n4096_slot_tiles_and_the_second_degree_tile():
    js = common.param_json("1M-1024-com")
    t = U.toy_t(js)
    G, sc = apsu_amd.HeContext(js), seal.SealContext(js)
    bins = (G.n // 5) * 5
    assert bins == 4095
    rng = np.random.default_rng(4096)
    B = [[] for _ in range(bins)]
    occupied = sorted(set([63, 64, 4031, bins - 1] + [int(s) for s in rng.choice(bins, 196, replace=False)]))
    for s in occupied:
        B[s] = U.distinct(rng, t, int(rng.integers(1, 40)))
    for s, c in zip((63, 64, 4031, bins - 1), (70, 65, 66, 69)):       # four bins reach into the second degree tile
        B[s] = U.distinct(rng, t, c)
    assert sum(len(x) > 64 for x in B) == 4 and max(len(x) for x in B) == 70
    b = G.build_bundle(1, 0, B)
    assert b.degree == 70
    check_export(G, sc, js, b, B, 0, compr=seal.COMPR_NONE, settings=(FULL,))
    check_export(G, sc, js, b, B, 0, compr=seal.COMPR_ZSTD, settings=(FULL,))
    G.close()
    sc.close()


def four_bundles(t):
    rng = np.random.default_rng(44)
    return {(i, c): [U.distinct(rng, t, (s + 3 * i + c) % 6) for s in range(60)] for i in (0, 1) for c in (0, 1)}


def test_whole_database(toy, tmp_path):
    js, G, sc, t = toy
    D = four_bundles(t)
    made = {k: G.build_bundle(k[0], k[1], B) for k, B in D.items()}
    scrambled = [made[(1, 0)], made[(0, 0)], made[(1, 1)], made[(0, 1)]]
    want = [G.save_bundle(made[k]).tobytes() for k in ((0, 0), (0, 1), (1, 0), (1, 1))]
    key = bytes((7 * i + 1) % 256 for i in range(32))
    hashed = [(2**64 - 1 - i, 3 * i) for i in range(7)]
    files = {}
    # stripped: the item count is the caller's; unstripped, ReceiverDB::Load wants it to be the number of hashed items
    for name, kw, count in (("stripped", dict(stripped=True), 123), ("full", dict(), 7), ("zstd", dict(compr=seal.COMPR_ZSTD), 7)):
        path = str(tmp_path / (name + ".db"))
        seal.export_saved_db(G, sc, path, scrambled, oprf_key=key, hashed_items=hashed, item_count=count, **kw)
        assert not os.path.exists(path + ".tmp")
        blob = open(path, "rb").read()
        files[name] = blob
        h = wire.parse_receiver_db_header(blob)
        assert (h["item_count"], h["bin_bundle_count"], h["stripped"], h["compressed"]) == (count, 4, name == "stripped", name == "zstd")
        assert h["oprf_key"] == key and h["hashed_items"] == hashed and json.loads(h["params_json"]) == json.loads(wire.psu_params_load(wire.psu_params_save(js)))
        G2, sc2, loaded = seal.load_reference_db(path)
        assert [(b.bundle_idx, b.cache_idx) for b in loaded] == [(0, 0), (0, 1), (1, 0), (1, 1)]
        assert [G2.save_bundle(b).tobytes() for b in loaded] == want
        G2.close()
        sc2.close()
    with pytest.raises(ValueError, match="item_count 123"):
        seal.export_saved_db(G, sc, str(tmp_path / "mismatch.db"), scrambled, oprf_key=key, hashed_items=hashed, item_count=123)
    with pytest.raises(ValueError, match="32 bytes"):
        seal.export_saved_db(G, sc, str(tmp_path / "key.db"), scrambled, oprf_key=key[:31], hashed_items=hashed, item_count=7)
    # a refused export leaves neither file
    path = str(tmp_path / "refused.db")
    with pytest.raises(ValueError, match=r"bin \d+"):
        seal.export_saved_db(G, sc, path, scrambled[:2] + [G.random_bundle(1, 2, 6, 3)] + scrambled[2:], oprf_key=key, hashed_items=hashed, item_count=7)
    assert not os.path.exists(path) and not os.path.exists(path + ".tmp")
    assert not os.path.exists(str(tmp_path / "mismatch.db")) and not os.path.exists(str(tmp_path / "mismatch.db.tmp"))
    # the same four BinBundles on a handle over the device list {0, 0}: a byte-identical file
    M = apsu_amd.MultiContext(js, [0, 0])
    for slot, k in ((1, (1, 1)), (0, (0, 1)), (1, (0, 0)), (0, (1, 0))):
        M.build_bundle(k[0], k[1], D[k], slot=slot)
    for name, kw, count in (("stripped", dict(stripped=True), 123), ("full", dict(), 7)):
        path = str(tmp_path / ("multi_" + name + ".db"))
        seal.export_saved_db(M, sc, path, oprf_key=key, hashed_items=hashed, item_count=count, **kw)
        assert open(path, "rb").read() == files[name]
    M.close()
