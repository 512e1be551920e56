"""GPU tier: apsu_he_bundles_merge and apsu_he_db_compact -- several BinBundles of one bundle index into one, without anybody's roots:
each input is decoded back to its bins' polynomials, the polynomials of equal slots are multiplied (k_bins_merge: the union of two
bins is the product of their polynomials) and the tail of the build re-encodes.  The contract is the update's: the image of
merge(build(A), build(B)) is byte-identical to that of build_bundle(A + B bin by bin), and every stored coefficient equals the
oracle's build of the union.  K = 8 output rows per wave (bin_merge.h: MERGE_K) decides the shapes below."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import apsu_amd
import common
import emu_lib
import test_bundle_merge_cpu as M
import test_gpu_bundle_update as U
from oracle import ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFF
K = 8
F = 5
SEED = bytes(range(1, 65))                                # 64 bytes: the querier's seed


def union(*parts):
    width = max(len(p) for p in parts)
    return [sum((list(p[s]) for p in parts if s < len(p)), []) for s in range(width)]


def bins_of(rng, t, counts, avoid=None):
    """per slot `counts[s]` distinct values, none of them in avoid[s]"""
    return [U.distinct(rng, t, c, avoid=avoid[s] if avoid else ()) for s, c in enumerate(counts)]


def check_merge(js, G, parts, bundle_idx=0, cache_idx=None, built=None):
    """merge(build(parts[0]), build(parts[1]), ..) -> (merged BinBundle, union bins), checked against the oracle's build of the union
    and, as an image, against build_bundle(union)"""
    p = ref.load_params(js)
    C = ref.RefContext.from_params(p)
    built = built or [G.build_bundle(bundle_idx, i, b) for i, b in enumerate(parts)]
    before = [G.save_bundle(b).tobytes() for b in built]
    merged = G.merge_bundles(built, cache_idx=cache_idx)
    want_cache = built[0].cache_idx if cache_idx is None else cache_idx
    assert (merged.bundle_idx, merged.cache_idx) == (bundle_idx, want_cache)
    all_bins = union(*parts)
    A, coeffs, flags = U.oracle_build(C, p["ps_low_degree"], all_bins)
    U.check_coeffs(G, C, p["ps_low_degree"], merged, coeffs, flags)
    rebuilt = G.build_bundle(bundle_idx, want_cache, all_bins)
    assert G.save_bundle(merged).tobytes() == G.save_bundle(rebuilt).tobytes(), "image differs from build_bundle(A + B)"
    assert [G.save_bundle(b).tobytes() for b in built] == before          # the inputs are only read
    return merged, all_bins


def test_two_tiles_with_different_loop_bounds_and_slots_that_are_not_bins():
    # n = 256, the engine's smallest degree with more than one tile: 255 bins, slot 255 holds the zero polynomial in both inputs
    js = common.toy_json(n=256)
    t = U.toy_t(js)
    rng = np.random.default_rng(41)
    G = apsu_amd.HeContext(js)
    for c in (3, 0, 10):
        ca, cb = [0] * 255, [0] * 255
        ca[5], cb[5] = 10 - c, c                           # tile 0: one bin at max_items - 1 - c against c, every other bin empty
        for s in range(64, 255):                           # tiles 1 .. 3: ragged, sums up to 6 (tile 2: up to 2)
            ca[s], cb[s] = int(rng.integers(0, 2 if 128 <= s < 192 else 4)), int(rng.integers(0, 2 if 128 <= s < 192 else 4))
        A = bins_of(rng, t, ca)
        merged, _ = check_merge(js, G, [A, bins_of(rng, t, cb, avoid=A)])
        assert merged.degree == 10
        counts = G.bin_counts(merged)
        assert (counts[255:] == NONE).all() and [int(v) for v in counts[:255]] == [x + y for x, y in zip(ca, cb)]
    G.close()


def test_row_block_boundaries_and_the_empty_input():
    js = common.toy_json(max_items=20)
    t = U.toy_t(js)
    rng = np.random.default_rng(42)
    G = apsu_amd.HeContext(js)
    # dA = 0: every bin of A is empty (the polynomial 1); the product is B, whichever side it is on
    B = U.rand_bins(rng, t, 60, 9)
    empty = [[] for _ in range(60)]
    m, _ = check_merge(js, G, [empty, B])
    assert G.save_bundle(m).tobytes() == G.save_bundle(G.build_bundle(0, 0, B)).tobytes()
    check_merge(js, G, [B, empty])
    # (dA, dB): dA < K with a partial last row block; dA + dB + 1 an exact multiple of K; two full blocks; one row beyond
    for da, db in ((3, 5), (3, 4), (7, 8), (8, 8)):
        assert ((da + db + 1) % K == 0) == ((da, db) in ((3, 4), (7, 8)))
        ca = [int(rng.integers(0, da + 1)) for _ in range(60)]
        cb = [int(rng.integers(0, db + 1)) for _ in range(60)]
        ca[9], cb[9], ca[33], cb[50] = da, db, da, db
        A = bins_of(rng, t, ca)
        m, _ = check_merge(js, G, [A, bins_of(rng, t, cb, avoid=A)], bundle_idx=1, cache_idx=7)
        assert m.degree == da + db
    G.close()


def test_double_roots_root_zero_and_the_layout_change():
    # toy ps_low_degree = 3: both inputs of degree <= 3 are all NTT-form; the product of degree 5 has the Paterson-Stockmeyer layout
    js = common.toy_json()
    t = U.toy_t(js)
    rng = np.random.default_rng(43)
    G = apsu_amd.HeContext(js)
    A = U.rand_bins(rng, t, 60, 3)
    B = [U.distinct(rng, t, int(rng.integers(0, 3)), avoid=a) for a in A]
    A[4], B[4] = [0, 17, 99], [17, 0]                     # root 0 and 17 on both sides: double roots
    A[8], B[8] = [5], [5]
    a, b = G.build_bundle(0, 0, A), G.build_bundle(0, 1, B)
    assert a.degree == 3 and b.degree <= 3
    m, bins = check_merge(js, G, [A, B], built=[a, b])
    assert m.degree == 5 and sorted(bins[4]) == [0, 0, 17, 17, 99]
    # a multiset: one removal takes out one occurrence, and the merged BinBundle updates like any other
    rem = [[] for _ in bins]
    rem[4], rem[8] = [17, 0], [5]
    U.check_update(js, G, m, bins, None, rem)
    G.close()


def test_three_way_merge_equals_both_pairwise_orders():
    js = common.toy_json()
    t = U.toy_t(js)
    rng = np.random.default_rng(44)
    G = apsu_amd.HeContext(js)
    A = U.rand_bins(rng, t, 60, 4, full_frac=0.2)
    B = [U.distinct(rng, t, int(rng.integers(0, 4)), avoid=a) for a in A]
    Cc = [U.distinct(rng, t, int(rng.integers(0, 4)), avoid=a + b) for a, b in zip(A, B)]
    gb = [G.build_bundle(0, i, x) for i, x in enumerate((A, B, Cc))]
    m3, _ = check_merge(js, G, [A, B, Cc], built=gb)
    ab_c = G.merge_bundles([G.merge_bundles(gb[:2]), gb[2]])
    a_bc = G.merge_bundles([gb[0], G.merge_bundles(gb[1:])])
    cba = G.merge_bundles(gb[::-1], cache_idx=0)
    img = G.save_bundle(m3).tobytes()
    assert G.save_bundle(ab_c).tobytes() == img and G.save_bundle(a_bc).tobytes() == img and G.save_bundle(cba).tobytes() == img
    G.close()


def test_wide_plain_modulus_takes_the_128_bit_sums():
    # a 33-bit plain modulus under 40-bit coefficient primes: q_0 > 2 t, so stored plaintexts decode, and t >= 2^32
    # (3 field elements of 32 bits per item: 5 would exceed the 128-bit item)
    js = common.toy_json(plain_bits=33, max_items=20, felts=3)
    t = U.toy_t(js)
    assert t >> 32 == 1
    rng = np.random.default_rng(45)
    G = apsu_amd.HeContext(js)
    ca = [int(rng.integers(0, 10)) for _ in range(60)]
    cb = [int(rng.integers(0, 10)) for _ in range(60)]
    ca[0], cb[0] = 9, 9
    A = [[t - 1 - i for i in range(c)] for c in ca]      # values next to t: products next to t^2
    B = [[t - 100 - i for i in range(c)] for c in cb]
    m, _ = check_merge(js, G, [A, B])
    assert m.degree == 18
    G.close()


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np, apsu_amd, common
G = apsu_amd.HeContext(common.toy_json())
src = np.load(sys.argv[3])
m = G.merge_bundles([G.load_bundle(src["a"]), G.load_bundle(src["b"])], cache_idx=0)
np.savez(sys.argv[4], degree=m.degree, image_format=G.save_bundle(m)[:256], **{"c%d" % d: G.bundle_coeff(m, d)[0] for d in range(m.degree + 1)})
"""


def test_merge_of_loaded_images_and_on_dense_rows(tmp_path):
    js = common.toy_json()
    t = U.toy_t(js)
    rng = np.random.default_rng(46)
    A = U.rand_bins(rng, t, 60, 5)
    B = [U.distinct(rng, t, int(rng.integers(0, 6)), avoid=a) for a in A]
    G = apsu_amd.HeContext(js)
    gb = [G.build_bundle(0, 0, A), G.build_bundle(0, 1, B)]
    m, _ = check_merge(js, G, [A, B], built=gb)
    images = [G.save_bundle(b) for b in gb]
    # a second context knows the images only (a loaded BinBundle carries its bundle index in the image)
    G2 = apsu_amd.HeContext(js)
    m2 = G2.merge_bundles([G2.load_bundle(im) for im in images], cache_idx=0)
    assert G2.save_bundle(m2).tobytes() == G.save_bundle(m).tobytes()
    G2.close()
    # dense 64-bit rows: APSU_HE_PACKED_ROWS is read when a context is created, so the merge runs in a fresh process
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "dense.npz")
    np.savez(src, a=images[0], b=images[1])
    env = dict(os.environ, APSU_HE_PACKED_ROWS="0")
    subprocess.run([sys.executable, "-c", CHILD, os.path.dirname(HERE), HERE, src, dst], env=env, check=True, timeout=120)
    got = np.load(dst)
    assert int(got["degree"]) == m.degree
    assert int(got["image_format"][8 + 16 + 88 + 8 + 28:][:4].view(np.uint32)[0]) == 0, "the child kept dense rows"
    for d in range(m.degree + 1):
        assert (got["c%d" % d] == G.bundle_coeff(m, d)[0]).all(), d
    G.close()


def test_merge_refusals_leave_no_handle_and_the_inputs_usable():
    js = common.toy_json()
    t = U.toy_t(js)
    rng = np.random.default_rng(47)
    G = apsu_amd.HeContext(js)
    A = U.rand_bins(rng, t, 60, 4, full_frac=0.0)
    B = [U.distinct(rng, t, int(rng.integers(0, 4)), avoid=a) for a in A]
    A[20], B[20] = U.distinct(rng, t, 6), U.distinct(rng, t, 5)             # 6 + 5 = 11 reaches max_items_per_bin
    A[40], B[40] = U.distinct(rng, t, 8), U.distinct(rng, t, 8)
    a, b = G.build_bundle(0, 0, A), G.build_bundle(0, 1, B)
    want = [G.save_bundle(x).tobytes() for x in (a, b)]
    with pytest.raises(ValueError, match=r"bin 20\b"):                      # the first slot is the one named
        G.merge_bundles([a, b])
    short = G.build_bundle(0, 2, B[:55])                                    # slots 55 .. 59 hold the zero polynomial here, bins there
    empty = G.build_bundle(0, 3, [[] for _ in range(60)])
    with pytest.raises(ValueError, match=r"slot 55\b"):
        G.merge_bundles([empty, short])
    other = G.build_bundle(1, 0, [[] for _ in range(60)])
    with pytest.raises(ValueError, match="bundle index"):
        G.merge_bundles([a, other])
    with pytest.raises(ValueError):
        G.merge_bundles([a])
    with pytest.raises(ValueError):
        G.merge_bundles([])
    assert [G.save_bundle(x).tobytes() for x in (a, b)] == want
    B[20], B[40] = B[20][:4], []                                            # 6 + 4 = 10: one below the bound
    check_merge(js, G, [A, B], built=[a, G.build_bundle(0, 1, B)])
    G.close()


def split_items(rng, t, x, starts):
    """per start bin two items for A and two for B (values distinct within a bin); the query values x[s .. s + 4] are A's first item at
    every third start bin, B's first item at the next, nobody's at the one after -> (items A, bins A, items B, bins B)"""
    bins = [[[] for _ in range(60)] for _ in range(2)]
    items = [[], []]
    for k, s in enumerate(starts):
        for side in range(2):
            for i in range(2):
                f = [U.distinct(rng, t, 1, avoid=bins[0][s + j] + bins[1][s + j] + [int(x[s + j])])[0] for j in range(F)]
                if i == 0 and side == k % 3:
                    f = [int(x[s + j]) for j in range(F)]
                items[side].append((s, f))
                for j in range(F):
                    bins[side][s + j].append(f[j])
    return items[0], bins[0], items[1], bins[1]


def test_merged_bundle_answers_queries_lookup_and_update():
    js = common.toy_json()
    S = common.make_scenario(js, {0: []})
    C, t, n = S.C, S.C.t, S.C.n
    rng = np.random.default_rng(48)
    items_a, A, items_b, B = split_items(rng, t, S.x[0], range(0, 60, F))
    G = apsu_amd.HeContext(js)
    merged, bins = check_merge(js, G, [A, B])
    # (i) ComputePowers + eval_bundles on the merged BinBundle: bit-identical to the oracle's evaluation of the union bins
    rk = G.upload_relin_keys(S.rk)
    pw = G.compute_powers([0], [[S.src[0][e] for e in S.sources]], rk)
    mask_vals = ref.fill_uniform(9, t, n)
    mask = C.encode(mask_vals)
    out = G.eval_bundles([merged], pw, rk, [mask])
    Aor, coeffs, flags = U.oracle_build(C, S.ps_low, bins)
    bundle = dict(bundle_idx=0, cache_idx=0, degree=len(coeffs) - 1, A=Aor, coeffs=coeffs, flags=flags, mask_vals=mask_vals, mask=mask)
    assert (out[0] == common.oracle_eval(S, common.oracle_powers(S), bundle)).all()
    # (ii) the engine's own querier: member slots decrypt to the mask alone, the others do not
    sk = G.keygen(SEED)
    _, _, rk2 = G.relin_keygen(sk, SEED)
    L, ns = G.first_chain_idx + 1, len(S.sources)
    dev = torch.zeros((ns, 2, L, n), dtype=torch.int64, device="cuda")
    G.query_create(sk, [0], S.x[0][None, :].copy(), dev.data_ptr(), seed=SEED)
    pw2 = G.compute_powers([0], [[dev.data_ptr() + s * 2 * L * n * 8 for s in range(ns)]], rk2, on_device=True)
    res = G.eval_bundles([merged], pw2, rk2, [mask])
    got = G.decrypt_decode(sk[0], res)[0].reshape(-1, n)[0]
    # (slots 60 .. 63 are not bins: the zero polynomial evaluates to 0 wherever it is asked)
    member = np.array([s >= 60 or int(S.x[0][s]) in bins[s] for s in range(n)])
    assert member[:10].all() and not member[10:15].any() and ((got == mask_vals) == member).all()
    # (iii) lookup finds entries that came from A and from B, and no others
    absent = [(s, [U.distinct(rng, t, 1, avoid=bins[s + j])[0] for j in range(F)]) for s in (0, 25)]
    entries = items_a[:4] + items_b[:4] + absent
    present, room = G.lookup([merged], entries)
    assert [bool(v) for v in present[0]] == [True] * 8 + [False] * 2
    assert int(room[0][0]) == 5
    # (iv) update: an item that came from B leaves; the result is the build of what remains
    s, f = items_b[1]
    rem = [[] for _ in bins]
    for j in range(F):
        rem[s + j] = [f[j]]
    up, left = U.check_update(js, G, merged, bins, None, rem)
    assert not G.lookup([up], [items_b[1]])[0][0][0] and G.lookup([up], [items_a[1]])[0][0][0]
    G.close()


def test_compact_four_sparse_and_one_full():
    js = common.toy_json()
    t = U.toy_t(js)
    rng = np.random.default_rng(49)
    G = apsu_amd.HeContext(js)
    full = [U.distinct(rng, t, 10) for _ in range(60)]                      # every bin at max_items_per_bin - 1: nothing fits
    parts = [full]
    for c in (3, 4, 4, 2):                                                   # 3 + 4 fit (< 11), + 4 = 11 does not, + 2 does
        avoid = union(*parts)
        parts.append([U.distinct(rng, t, int(rng.integers(0, c + 1)) if s != 12 else c, avoid=avoid[s]) for s in range(60)])
    order = [1, 0, 2, 3, 4]                                                  # the full one second
    parts = [parts[i] for i in order]
    gb = [G.build_bundle(0, 2 * i + 1, b) for i, b in enumerate(parts)]
    counts = np.stack([G.bin_counts(b) for b in gb])
    res = G.compact(0, gb)
    group = [int(g) for g in res.group]
    assert group == [0, 1, 0, 2, 0]
    assert M.run_plan(emu_lib.load(), counts[:, :60], 11)[0] == group          # the groups are the planner's
    degrees = [max(len(b) for b in union(*[parts[i] for i in range(5) if group[i] == g])) for g in range(3)]
    assert M.plan_errors([[int(v) for v in c] for c in counts], 11, group, degrees) == []
    assert len(res.merged) == 3 and res.merged[1] is None and res.merged[2] is None          # groups of one: untouched
    m = res.merged[0]
    assert (m.bundle_idx, m.cache_idx) == (0, gb[0].cache_idx)
    want = G.build_bundle(0, gb[0].cache_idx, union(parts[0], parts[2], parts[4]))
    assert G.save_bundle(m).tobytes() == G.save_bundle(want).tobytes()
    # a second compact on the result merges nothing
    after = [m, gb[1], gb[3]]
    again = G.compact(0, after)
    assert [int(g) for g in again.group] == [0, 1, 2] and again.merged == [None, None, None]
    # refused: out of cache order, another bundle index
    with pytest.raises(ValueError):
        G.compact(0, [gb[1], gb[0]])
    with pytest.raises(ValueError):
        G.compact(1, gb)
    assert G.compact(0, []).merged == []
    G.close()
