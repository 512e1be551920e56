"""GPU tier: apsu_he_bundle_adopt and apsu_he_db_rebase -- the BinBundles of one context moved to a context with other parameters of the
same ring, plain modulus and table and item geometry: the coefficient half of the source's decode, then the destination's own build
tail; a split in the source first where the destination allows fewer items per bin.  The contract is the build's: the image in the
destination is byte-identical to that of dst.build_bundle of the same bins."""
import json

import numpy as np
import pytest

import apsu_amd
import common
import split_model as M
import test_gpu_bundle_update as U

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


def image(G, b):
    return G.save_bundle(b).tobytes()


def check_adopt(src, dst, bins, bundle_idx=0, cache_idx=2, new_cache=None):
    b = src.build_bundle(bundle_idx, cache_idx, bins)
    before = image(src, b)
    moved = dst.adopt_bundle(src, b, cache_idx=new_cache)
    ci = cache_idx if new_cache is None else new_cache
    assert (moved.bundle_idx, moved.cache_idx, moved.degree) == (bundle_idx, ci, b.degree)
    assert image(dst, moved) == image(dst, dst.build_bundle(bundle_idx, ci, bins)), "image differs from the destination's own build"
    assert image(src, b) == before                          # the input is only read
    return moved


PAIRS = [pytest.param(dict(), dict(coeff_bits=(50, 50, 40)), id="coefficient-primes"),
         pytest.param(dict(ps_low=3), dict(ps_low=0, query_powers=(1,)), id="ps_low-3-0"),
         pytest.param(dict(ps_low=3), dict(ps_low=5, query_powers=(1, 2, 3, 4, 5, 6)), id="ps_low-3-5"),
         pytest.param(dict(max_items=11), dict(max_items=7), id="max_items-11-7")]


@pytest.mark.parametrize("a,b", PAIRS)
def test_adopt_image_equals_the_destinations_build_both_directions(a, b):
    ja, jb = common.toy_json(**a), common.toy_json(**b)
    t = U.toy_t(ja)
    rng = np.random.default_rng(61)
    A, B = apsu_amd.HeContext(ja), apsu_amd.HeContext(jb)
    most = min(json.loads(ja)["table_params"]["max_items_per_bin"], json.loads(jb)["table_params"]["max_items_per_bin"])
    for deg in (most, 3, 0):
        bins = U.rand_bins(rng, t, 60, deg, full_frac=0.2)
        bins[3], bins[7] = [], ([0] if deg else [])
        if deg:
            bins[11] = U.distinct(rng, t, deg)
        check_adopt(A, B, bins)
        check_adopt(B, A, bins, bundle_idx=1, new_cache=9)
    A.close()
    B.close()


def test_adopt_a_bundle_with_an_unlifted_monomial():
    # every slot of exactly h = 4 items: a_4 is the all-ones vector, a constant plaintext, which the source stores un-lifted; the
    # destination (ps_low 0) stores it in NTT form, and on the way back it is un-lifted again
    ja, jb = common.toy_json(), common.toy_json(ps_low=0, query_powers=(1,))
    t = U.toy_t(ja)
    rng = np.random.default_rng(62)
    A, B = apsu_amd.HeContext(ja), apsu_amd.HeContext(jb)
    bins = [U.distinct(rng, t, 4) for _ in range(64)]
    moved = check_adopt(A, B, bins)
    back = A.adopt_bundle(B, moved)
    assert image(A, back) == image(A, A.build_bundle(0, 2, bins))
    A.close()
    B.close()


def test_rebase_1M_512_com_to_cmp_splits_the_full_bundle():
    src, dst = apsu_amd.HeContext(common.param_json("1M-512-com")), apsu_amd.HeContext(common.param_json("1M-512-cmp"))
    t = src.t
    rng = np.random.default_rng(63)
    full = [[] for _ in range(30)]
    for s in range(0, 30, 3):
        full[s] = U.distinct(rng, t, int(rng.integers(1, 100)))
    full[9] = U.distinct(rng, t, 227)                       # one bin at the source's bound: two parts, every bin below 128
    small = [U.distinct(rng, t, int(rng.integers(0, 20))) for _ in range(24)]
    inputs = [src.build_bundle(0, 0, small), src.build_bundle(0, 1, full), src.build_bundle(1, 0, small)]
    moved, origin = dst.rebase_from(src, inputs)
    assert origin == [0, 1, 1, 2]
    assert [(m.bundle_idx, m.cache_idx) for m in moved] == [(0, 0), (0, 1), (0, 2), (1, 0)]      # dense per bundle index, by position
    parts = M.split_bins(full, 2)
    want = [small, parts[0], parts[1], small]
    for m, bins in zip(moved, want):
        assert image(dst, m) == image(dst, dst.build_bundle(m.bundle_idx, m.cache_idx, bins))
        counts = dst.bin_counts(m)
        assert max(int(c) for c in counts if c != NONE) < 128
    rep = dst.self_test(moved, seed=bytes(range(64)))
    assert rep.mismatches == 0 and rep.bundles == 4 and rep.min_budget > 0
    src.close()
    dst.close()


def test_rebase_256K_2048_cmp_to_com_then_compact():
    src, dst = apsu_amd.HeContext(common.param_json("256K-2048-cmp")), apsu_amd.HeContext(common.param_json("256K-2048-com"))
    t = src.t
    rng = np.random.default_rng(64)
    A = [U.distinct(rng, t, int(rng.integers(0, 20))) for _ in range(20)]
    B = [U.distinct(rng, t, int(rng.integers(0, 20)), avoid=a) for a in A]
    A[4] = U.distinct(rng, t, 31, avoid=B[4])              # the source's bound; 31 + 19 < 51
    inputs = [src.build_bundle(2, 0, A), src.build_bundle(2, 1, B)]
    moved, origin = dst.rebase_from(src, inputs)
    assert origin == [0, 1] and [m.cache_idx for m in moved] == [0, 1]
    for m, bins in zip(moved, (A, B)):
        assert image(dst, m) == image(dst, dst.build_bundle(2, m.cache_idx, bins))
    res = dst.compact(2, moved)                             # the destination allows fuller bins: the existing call merges them
    merged = [m for m in res.merged if m is not None]
    assert len(merged) == 1
    assert image(dst, merged[0]) == image(dst, dst.build_bundle(2, 0, [a + b for a, b in zip(A, B)]))
    src.close()
    dst.close()


def test_adopt_and_rebase_refusals():
    base = apsu_amd.HeContext(common.toy_json())
    t = U.toy_t()
    rng = np.random.default_rng(65)
    bins = U.rand_bins(rng, t, 60, 10)
    bins[1] = U.distinct(rng, t, 10)
    b = base.build_bundle(0, 0, bins)
    for kw, why in ((dict(plain_bits=18), "plain_modulus differs"), (dict(n=256), "poly_modulus_degree differs"),
                    (dict(felts=6), "felts_per_item differs"), (dict(table_mult=3), "table_size differs")):
        other = apsu_amd.HeContext(common.toy_json(**kw))
        with pytest.raises(ValueError, match=why):
            other.adopt_bundle(base, b)
        with pytest.raises(ValueError, match=why):
            other.rebase_from(base, [b])
        other.close()
    small = apsu_amd.HeContext(common.toy_json(max_items=7))
    with pytest.raises(ValueError, match="degree 10, above the destination's max_items_per_bin = 7: split it into 2 parts"):
        small.adopt_bundle(base, b)
    # all or nothing: the last BinBundle needs a split and does not split; nothing comes back, and both contexts go on
    good = base.build_bundle(0, 1, U.rand_bins(rng, t, 60, 5))
    rnd = base.random_bundle(0, 2, 9, 7)
    with pytest.raises(ValueError, match="does not split into linear factors"):
        small.rebase_from(base, [good, b, rnd])
    moved, origin = small.rebase_from(base, [good, b])
    assert origin == [0, 1, 1] and [m.cache_idx for m in moved] == [0, 1, 2]
    parts = M.split_bins(bins, 2)
    assert image(small, moved[1]) == image(small, small.build_bundle(0, 1, parts[0]))
    assert image(small, moved[2]) == image(small, small.build_bundle(0, 2, parts[1]))
    small.close()
    base.close()
