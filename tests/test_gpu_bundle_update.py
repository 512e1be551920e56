"""GPU tier: apsu_he_bundle_update -- insert and remove items in a resident BinBundle (ReceiverDB::insert_or_assign / remove ->
BinBundle::multi_insert / try_multi_remove -> regen_cache, receiver_db.cpp:330-433) without its roots: the stored coefficients are
decoded back to the bins' polynomials, each named bin is multiplied / divided by (x - r) in one wave (k_bins_update), and the
result is re-encoded by the tail of the build.  Every case checks the updated BinBundle (i) coefficient by coefficient against the
oracle's build of the updated bins B' and (ii) byte for byte, as an image, against build_bundle(B').

The image of build_bundle(base_bins()) is also held to the bytes the build produced before its tail was factored out
(tests/golden/bundle_update_build_image.npy), made at that commit with
    python -c "import sys; sys.path.insert(0, 'tests'); import numpy as np, apsu_amd, common, test_gpu_bundle_update as T; \
G = apsu_amd.HeContext(common.toy_json()); np.save('tests/golden/bundle_update_build_image.npy', G.save_bundle(G.build_bundle(0, 0, T.base_bins())))"
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import apsu_amd
import common
from oracle import ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def oracle_build(C, ps_low, bins):
    """per-bin monic polynomial with the bin's items as roots (interpolate.cpp:63-80), coefficient d of every bin batched into one
    plaintext in the BinBundle layout (bin_bundle.cpp:395-430)"""
    n = C.n
    deg = max([len(b) for b in bins] + [0])
    A = np.zeros((deg + 1, n), dtype=np.uint64)
    for s, b in enumerate(bins):
        p = C.polyn_with_roots(np.array(b, dtype=np.uint64)) if len(b) else np.array([1], dtype=np.uint64)
        A[:len(p), s] = p
    pci = C.plain_chain_idx(ps_low)
    coeffs, flags = [], []
    for d in range(deg + 1):
        enc = C.encode(A[d])
        ntt = ref.coeff_is_ntt(ps_low, d)
        coeffs.append(C.plain_lift_ntt(enc, pci) if ntt else enc)
        flags.append(ntt)
    return A, coeffs, flags


def check_coeffs(G, C, ps, gb, coeffs, flags, degrees=None):
    """every stored coefficient of gb equals the oracle's (the comparison of the build tests)"""
    deg = len(coeffs) - 1
    assert gb.degree == deg
    use_ps = ps > 1 and ps < deg
    high = C.clamp(1)
    for d in (range(deg + 1) if degrees is None else degrees):
        if d > 0 and not flags[d] and not use_ps:
            continue
        got, kind = G.bundle_coeff(gb, d)
        if d == 0:
            assert kind == 0 and (got == coeffs[0]).all()
        elif flags[d]:
            assert kind == 1 and (got == coeffs[d]).all(), "NTT-form coefficient %d" % d
        else:
            exp = C.plain_lift_ntt(coeffs[d], high)
            if np.count_nonzero(coeffs[d]) == 1:              # monomial shortcut of multiply_plain: no lift
                exp = np.tile(coeffs[d], (high + 1, 1)).reshape(1, high + 1, C.n).copy()
                C.transform_to_ntt(exp, high)
                exp = exp[0]
            assert kind == 2 and (got == exp).all(), "coefficient-form coefficient %d" % d


def rand_bins(rng, t, n_bins, max_count, full_frac=0.3):
    bins = []
    for s in range(n_bins):
        c = max_count if rng.random() < full_frac else int(rng.integers(0, max_count + 1))
        bins.append([int(v) for v in rng.choice(t - 1, size=c, replace=False) + 1])
    return bins


def distinct(rng, t, count, avoid=()):
    out = []
    while len(out) < count:
        v = int(rng.integers(1, t))
        if v not in out and v not in avoid:
            out.append(v)
    return out


def toy_t(js=None):
    return ref.RefContext.from_params(ref.load_params(js or common.toy_json())).t


def base_bins():
    """ragged toy bins: 60 of 64 slots used, one empty bin, one holding root 0, largest bin 10 of max_items_per_bin = 11"""
    rng = np.random.default_rng(21)
    t = toy_t()
    bins = rand_bins(rng, t, 60, 10)
    bins[3] = []
    bins[7] = [0]
    bins[11] = distinct(rng, t, 10)
    return bins


def apply_update(bins, inserts, removes):
    """B': removals first (one occurrence per listed value), then insertions"""
    out = [list(b) for b in bins]
    for s, r in enumerate(removes or []):
        for v in r:
            out[s].remove(v)
    for s, a in enumerate(inserts or []):
        while len(out) <= s:
            out.append([])
        out[s].extend(a)
    return out


def check_update(js, G, old, bins, inserts, removes, degrees=None):
    """update `old` (a BinBundle holding `bins`) -> (updated BinBundle, B'), checked against the oracle and against the build of B'"""
    p = ref.load_params(js)
    C = ref.RefContext.from_params(p)
    new_bins = apply_update(bins, inserts, removes)
    up = G.update_bundle(old, inserts=inserts, removes=removes)
    assert (up.bundle_idx, up.cache_idx) == (old.bundle_idx, old.cache_idx)
    A, coeffs, flags = oracle_build(C, p["ps_low_degree"], new_bins)
    check_coeffs(G, C, p["ps_low_degree"], up, coeffs, flags, degrees)                                         # (i)
    rebuilt = G.build_bundle(old.bundle_idx, old.cache_idx, new_bins)
    assert G.save_bundle(up).tobytes() == G.save_bundle(rebuilt).tobytes(), "image differs from build_bundle(B')"     # (ii)
    return up, new_bins


def mixed_lists(rng, t, bins, cap):
    """inserts in some bins, removes in others, both in a few; no bin grows beyond `cap`"""
    ins, rem = [[] for _ in bins], [[] for _ in bins]
    for s, b in enumerate(bins):
        kind = s % 5
        if kind in (1, 3) and b:
            rem[s] = [b[int(rng.integers(0, len(b)))]]
        if kind in (2, 3) and len(b) - len(rem[s]) < cap:
            ins[s] = distinct(rng, t, 1, avoid=b)
    return ins, rem


def test_build_image_is_what_it_was_before_the_tail_was_shared():
    js = common.toy_json()
    G = apsu_amd.HeContext(js)
    img = G.save_bundle(G.build_bundle(0, 0, base_bins()))
    want = np.load(os.path.join(HERE, "golden", "bundle_update_build_image.npy"))
    assert img.tobytes() == want.tobytes()
    G.close()


def test_update_ragged_bins_keeps_the_degree():
    js = common.toy_json()
    rng = np.random.default_rng(22)
    t = toy_t()
    bins = base_bins()
    G = apsu_amd.HeContext(js)
    old = G.build_bundle(0, 0, bins)
    ins, rem = mixed_lists(rng, t, bins, 10)
    ins[3] = distinct(rng, t, 2)                          # into the empty bin (polynomial 1)
    rem[7], ins[7] = [0], [0, 5]                          # root 0 out and in again, next to another one
    before = G.save_bundle(old).tobytes()
    up, new_bins = check_update(js, G, old, bins, ins, rem)
    assert up.degree == old.degree == 10
    assert G.save_bundle(old).tobytes() == before         # `old` is only read
    # the updated BinBundle is a BinBundle like any other: update it again, back to where it started
    back, bins2 = check_update(js, G, up, new_bins, rem, ins)
    assert sorted(map(sorted, bins2)) == sorted(map(sorted, bins))
    assert G.save_bundle(back).tobytes() == before
    G.close()


def test_update_changes_the_degree():
    js = common.toy_json()
    rng = np.random.default_rng(23)
    t = toy_t()
    G = apsu_amd.HeContext(js)
    bins = base_bins()
    old = G.build_bundle(1, 0, bins)
    ins = [[] for _ in bins]
    ins[11] = distinct(rng, t, 1, avoid=bins[11])          # 10 -> 11 = max_items_per_bin
    up, _ = check_update(js, G, old, bins, ins, None)
    assert up.degree == 11
    bins = rand_bins(rng, t, 60, 7)
    bins[20] = distinct(rng, t, 11)                        # the one full bin
    old = G.build_bundle(1, 0, bins)
    rem = [[] for _ in bins]
    rem[20] = bins[20][2:6]
    up, _ = check_update(js, G, old, bins, None, rem)
    assert up.degree == 7
    G.close()


def test_update_crosses_ps_low_degree_both_ways():
    # toy ps_low_degree = 3: at degree 3 everything is NTT-form at plain level 1 ... use_ps and `lifted` appear at degree 5
    js = common.toy_json()
    rng = np.random.default_rng(24)
    t = toy_t()
    G = apsu_amd.HeContext(js)
    bins = rand_bins(rng, t, 60, 3)
    bins[5] = distinct(rng, t, 3)
    old = G.build_bundle(0, 0, bins)
    ins = [[] for _ in bins]
    ins[5] = distinct(rng, t, 2, avoid=bins[5])
    up, bins5 = check_update(js, G, old, bins, ins, None)
    assert (old.degree, up.degree) == (3, 5)
    down, _ = check_update(js, G, up, bins5, None, ins)
    assert down.degree == 3
    assert G.save_bundle(down).tobytes() == G.save_bundle(old).tobytes()
    G.close()


def test_update_into_and_out_of_the_monomial_shortcut():
    # every slot of exactly h = 4 (then 2h = 8) items: a_4 (a_8) is the all-ones vector, a constant plaintext, stored un-lifted
    js = common.toy_json()
    rng = np.random.default_rng(25)
    t = toy_t()
    G = apsu_amd.HeContext(js)
    bins = [distinct(rng, t, int(rng.integers(0, 5))) for _ in range(64)]
    bins[0] = distinct(rng, t, 4)
    old = G.build_bundle(0, 0, bins)
    ins = [distinct(rng, t, 4 - len(b), avoid=b) for b in bins]
    up4, bins4 = check_update(js, G, old, bins, ins, None)
    assert up4.degree == 4 and all(len(b) == 4 for b in bins4)
    ins = [distinct(rng, t, 4, avoid=b) for b in bins4]
    up8, bins8 = check_update(js, G, up4, bins4, ins, None)
    assert up8.degree == 8
    rem = [b[:int(rng.integers(0, 9))] for b in bins8]
    rem[1] = []
    ragged, _ = check_update(js, G, up8, bins8, None, rem)
    assert ragged.degree == 8
    G.close()


def test_update_across_register_slot_boundaries():
    js = common.toy_json(ps_low=0, max_items=210, query_powers=(1,))
    rng = np.random.default_rng(26)
    t = toy_t(js)
    before, after = [63, 64, 65, 200, 0, 1, 129], [64, 63, 66, 128, 1, 0, 127]
    bins = [distinct(rng, t, c) for c in before]
    ins, rem = [], []
    for b, c0, c1 in zip(bins, before, after):
        # the appropriate mix: a few more removals than needed, made up by insertions
        n_rem = min(c0, max(c0 - c1, 0) + 2)
        rem.append([b[int(i)] for i in rng.choice(c0, size=n_rem, replace=False)] if n_rem else [])
        ins.append(distinct(rng, t, c1 - (c0 - n_rem), avoid=b))
    G = apsu_amd.HeContext(js)
    old = G.build_bundle(0, 0, bins)
    up, new_bins = check_update(js, G, old, bins, ins, rem)
    assert [len(b) for b in new_bins] == after and up.degree == 128
    G.close()


def test_update_takes_the_serial_fallback_beyond_8192_coefficients():
    """(about 20 s, nearly all of it in the two thread-per-bin BUILDS of 8299-item bins that the case needs for `old` and for the
    image of B' -- the cost of the same size in the build tests; the update itself takes milliseconds)"""
    js = common.toy_json(ps_low=0, max_items=8300, query_powers=(1,))
    rng = np.random.default_rng(27)
    t = toy_t(js)
    pool = [int(v) for v in rng.choice(t - 1, size=8299 + 8297 + 8, replace=False) + 1]
    bins = [pool[:8299], pool[8299:8299 + 8297], pool[-8:-5], pool[-5:-4]]
    ins = [[], pool[-4:-2], pool[-2:-1], []]
    rem = [[bins[0][4000]], [], [bins[2][1]], [bins[3][0]]]
    G = apsu_amd.HeContext(js)
    old = G.build_bundle(0, 0, bins)
    up, new_bins = check_update(js, G, old, bins, ins, rem, degrees=[0, 1, 2, 63, 64, 4000, 8191, 8192, 8297, 8298, 8299])
    assert [len(b) for b in new_bins] == [8298, 8299, 3, 0] and up.degree == 8299
    G.close()


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np, apsu_amd, common, test_gpu_bundle_update as T
G = apsu_amd.HeContext(common.toy_json())
old = G.load_bundle(np.load(sys.argv[3]))
ins, rem = T.no_roots_lists()
up = G.update_bundle(old, inserts=ins, removes=rem)
np.savez(sys.argv[4], degree=up.degree, image_format=G.save_bundle(up)[:256], **{"c%d" % d: G.bundle_coeff(up, d)[0] for d in range(up.degree + 1)})
"""


def no_roots_lists():
    rng = np.random.default_rng(28)
    ins, rem = mixed_lists(rng, toy_t(), base_bins(), 10)
    return ins, rem


def test_update_of_a_bundle_whose_roots_this_process_never_saw(tmp_path):
    js = common.toy_json()
    bins = base_bins()
    ins, rem = no_roots_lists()
    G = apsu_amd.HeContext(js)
    old = G.build_bundle(0, 0, bins)
    up, _ = check_update(js, G, old, bins, ins, rem)
    image = G.save_bundle(old)
    # a second context knows the image only
    G2 = apsu_amd.HeContext(js)
    up2 = G2.update_bundle(G2.load_bundle(image), inserts=ins, removes=rem)
    assert G2.save_bundle(up2).tobytes() == G.save_bundle(up).tobytes()
    G2.close()
    # dense 64-bit rows: APSU_HE_PACKED_ROWS is read when a context is created, so the update runs in a fresh process
    src, dst = str(tmp_path / "old.npy"), str(tmp_path / "dense.npz")
    np.save(src, image)
    env = dict(os.environ, APSU_HE_PACKED_ROWS="0")
    subprocess.run([sys.executable, "-c", CHILD, os.path.dirname(HERE), HERE, src, dst], env=env, check=True, timeout=120)
    got = np.load(dst)
    assert int(got["degree"]) == up.degree
    assert int(got["image_format"][8 + 16 + 88 + 8 + 28:][:4].view(np.uint32)[0]) == 0, "the child kept dense rows"
    for d in range(up.degree + 1):
        assert (got["c%d" % d] == G.bundle_coeff(up, d)[0]).all(), d
    G.close()


def test_update_1M_flips_the_membership_pattern():
    rng = np.random.default_rng(8)
    js = common.param_json("1M-1024-com")
    S = common.make_scenario(js, {0: []})
    C = S.C
    n_bins = S.p["items_per_bundle"] * S.p["felts_per_item"]
    bins = rand_bins(rng, C.t, n_bins, 60, full_frac=0.1)
    for s in range(0, n_bins, 2):                         # the query value is a member of every other bin
        if bins[s]:
            bins[s][0] = int(S.x[0][s])
    member = [s % 2 == 0 and bool(bins[s]) for s in range(n_bins)]
    for s in range(n_bins):                                # (a draw may have hit the query value by chance: once in a member bin, never elsewhere)
        bins[s] = bins[s][:1 if member[s] else 0] + [v for v in bins[s][1 if member[s] else 0:] if v != int(S.x[0][s])]
    rem = [[int(S.x[0][s])] if member[s] else [] for s in range(n_bins)]
    ins = [[] if member[s] else [int(S.x[0][s])] for s in range(n_bins)]
    new_bins = apply_update(bins, ins, rem)
    G = apsu_amd.HeContext(js)
    old = G.build_bundle(0, 0, bins)
    up = G.update_bundle(old, inserts=ins, removes=rem)
    A, coeffs, flags = oracle_build(C, S.ps_low, new_bins)
    assert up.degree == len(coeffs) - 1
    assert G.save_bundle(up).tobytes() == G.save_bundle(G.build_bundle(0, 0, new_bins)).tobytes()
    rk = G.upload_relin_keys(S.rk)
    pw = G.compute_powers([0], [[S.src[0][e] for e in S.sources]], rk)
    mask_vals = ref.fill_uniform(9, C.t, C.n)
    mask = C.encode(mask_vals)
    out = G.eval_bundles([up], pw, rk, [mask])
    bundle = dict(bundle_idx=0, cache_idx=0, degree=len(coeffs) - 1, A=A, coeffs=coeffs, flags=flags, mask_vals=mask_vals, mask=mask)
    assert (out[0] == common.oracle_eval(S, common.oracle_powers(S), bundle)).all()
    got = C.decode(C.decrypt(S.sk, out[0], 0)[0])
    now_member = np.array([not m for m in member])
    assert ((got == mask_vals)[:n_bins] == now_member).all()   # the mask alone exactly at the new member slots
    G.close()


def test_update_refusals():
    js = common.toy_json()
    S = common.make_scenario(js, {0: []})
    t = toy_t()
    bins = base_bins()
    G = apsu_amd.HeContext(js)
    old = G.build_bundle(0, 0, bins)
    rk = G.upload_relin_keys(S.rk)
    pw = G.compute_powers([0], [[S.src[0][e] for e in S.sources]], rk)
    mask = S.C.encode(ref.fill_uniform(9, S.C.t, S.C.n))
    want = G.eval_bundles([old], pw, rk, [mask]).copy()
    absent = distinct(np.random.default_rng(29), t, 1, avoid=bins[9] + bins[30])[0]
    rem = [[] for _ in bins]
    rem[30] = [bins[30][0], absent] if bins[30] else [absent]
    rem[9] = [absent]                                      # the lowest slot that fails is the one reported
    with pytest.raises(ValueError, match=r"bin 9\b.*\b%d\b" % absent):
        G.update_bundle(old, removes=rem)
    assert (G.eval_bundles([old], pw, rk, [mask]) == want).all()
    one = lambda s, v: [[]] * s + [v]
    with pytest.raises(ValueError):
        G.update_bundle(old, inserts=one(2, [t]))                           # unreduced field element
    with pytest.raises(ValueError):
        G.update_bundle(old, removes=one(2, [t + 5]))
    with pytest.raises(ValueError):
        G.update_bundle(old, inserts=one(11, distinct(np.random.default_rng(1), t, 2, avoid=bins[11])))   # 10 + 2 > max_items_per_bin
    with pytest.raises(ValueError):
        G.update_bundle(old, inserts=one(61, [5]))                          # slots 60 .. 63 hold the zero polynomial: not bins
    with pytest.raises(ValueError):
        G.update_bundle(old, inserts=one(64, [5]))                          # more bins than batching slots
    assert (G.eval_bundles([old], pw, rk, [mask]) == want).all()
    G.close()


def test_update_through_the_multi_device_handle(tmp_path):
    js = common.toy_json()
    S = common.make_scenario(js, {0: [], 1: []})
    t = toy_t()
    bins = base_bins()
    ins, rem = mixed_lists(np.random.default_rng(30), t, bins, 10)
    G = apsu_amd.HeContext(js)
    rk = G.upload_relin_keys(S.rk)
    pw = G.compute_powers(S.bundle_indices, [[S.src[b][e] for e in S.sources] for b in S.bundle_indices], rk)
    gb = [G.random_bundle(0, 0, 9, 77), G.build_bundle(1, 0, bins), G.random_bundle(1, 1, 11, 78)]
    masks = [S.C.encode(ref.fill_uniform(40 + i, S.C.t, S.C.n)) for i in range(3)]
    before = G.eval_bundles(gb, pw, rk, masks).copy()
    path = str(tmp_path / "db.apsuhe")
    G.save_db_file(path, gb)
    M = apsu_amd.MultiContext(js, [0])
    M.upload_relin_keys(S.rk)
    assert M.load_db_file(path) == 3
    flat = [S.src[b][e] for b in range(S.p["bundle_idx_count"]) for e in S.sources]
    assert (M.eval_all(flat, masks, G.n) == before).all()
    M.update_bundle(1, inserts=ins, removes=rem)
    single = G.eval_bundles([G.update_bundle(gb[1], inserts=ins, removes=rem)], pw, rk, [masks[1]])
    after = M.eval_all(flat, masks, G.n)
    assert (after[1] == single[0]).all() and not (after[1] == before[1]).all()
    assert (after[0] == before[0]).all() and (after[2] == before[2]).all()
    with pytest.raises(ValueError):
        M.update_bundle(3, inserts=ins)                    # no such id
    M.close()
    G.close()
