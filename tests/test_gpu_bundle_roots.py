"""GPU tier: apsu_he_bundle_bins -- the items of a resident BinBundle read back from its polynomials (apsu_amd/csrc/bin_roots.h,
kernels_roots.hip: k_bin_roots, persistent over the cosets of the transform's points, and k_roots_mult).  The contract: for
b = build_bundle(B), any update or merge of such BinBundles, and the same BinBundle loaded from an image, bins(b) equals B bin by bin as
a sorted multiset, build_bundle(bins(b)) has a byte-identical image, and the counts are bin_counts's.  Everything is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import apsu_amd
import common
import test_gpu_bundle_update as U
from apsu_amd import engine as E

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFF
KERNEL, COMPOSED = 1, 2


def as_lists(bins):
    return [None if b is None else [int(v) for v in b] for b in bins]


def want_lists(B, n):
    return [sorted(B[s]) if s < len(B) else None for s in range(n)]


def toy_bins(t):
    """60 bins of the toy ring: ragged counts 0 .. 10, double and triple roots, the root 0 once and twice, the largest field element"""
    rng = np.random.default_rng(61)
    B = [U.distinct(rng, t, s % 11) for s in range(60)]
    B[4] = [0, 0, 17, 17, 99]
    B[8] = [5, 5, 5]
    B[15] = [0]
    B[21] = [t - 1]
    B[33] = sorted(U.distinct(rng, t, 8) + [t - 1, t - 1])
    return B


def check_bins(G, b, B, forms=(0,)):
    """bins(b) == B, counts == bin_counts, build_bundle(bins(b)) image-identical to b"""
    n = G.n
    counts = G.bin_counts(b)
    assert [int(c) for c in counts] == [len(B[s]) if s < len(B) else NONE for s in range(n)]
    image = G.save_bundle(b).tobytes()
    got = None
    for form in forms:
        got = as_lists(G.bins(b, _form=form))
        assert got == want_lists(B, n), "form %d" % form
    assert G.save_bundle(b).tobytes() == image                        # the BinBundle is only read
    rebuilt = G.build_bundle(b.bundle_idx, b.cache_idx, [x for x in got if x is not None])
    assert G.save_bundle(rebuilt).tobytes() == image, "build_bundle(bins(b)) differs from b"
    return got


def test_toy_ring_ragged_bins_multiple_roots_and_slots_that_are_not_bins():
    js = common.toy_json()
    t = U.toy_t(js)
    G = apsu_amd.HeContext(js)
    B = toy_bins(t)
    b = G.build_bundle(1, 3, B)
    assert b.degree == 10
    got = check_bins(G, b, B, forms=(0, KERNEL, COMPOSED))            # the persistent kernel and the per-coset composition agree
    assert got[60:] == [None] * 4 and got[4] == [0, 0, 17, 17, 99] and got[8] == [5, 5, 5] and got[0] == []
    dec, search, mult = G.bins_times()
    assert dec > 0 and search > 0 and mult >= 0
    G.close()


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np, apsu_amd, common
G = apsu_amd.HeContext(common.toy_json())
b = G.load_bundle(np.load(sys.argv[3])["image"])
bins = G.bins(b)
np.savez(sys.argv[4], image_format=G.save_bundle(b)[:256], counts=G.bin_counts(b), **{"b%d" % s: v for s, v in enumerate(bins) if v is not None})
"""


def test_toy_ring_on_dense_rows(tmp_path):
    js = common.toy_json()
    t = U.toy_t(js)
    G = apsu_amd.HeContext(js)
    B = toy_bins(t)
    image = G.save_bundle(G.build_bundle(0, 0, B))
    G.close()
    # dense 64-bit rows: APSU_HE_PACKED_ROWS is read when a context is created, so the call runs in a fresh process
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "bins.npz")
    np.savez(src, image=image)
    env = dict(os.environ, APSU_HE_PACKED_ROWS="0")
    subprocess.run([sys.executable, "-c", CHILD, os.path.dirname(HERE), HERE, src, dst], env=env, check=True, timeout=120)
    got = np.load(dst)
    assert int(got["image_format"][8 + 16 + 88 + 8 + 28:][:4].view(np.uint32)[0]) == 0, "the child kept dense rows"
    assert [int(c) for c in got["counts"]] == [len(x) for x in B] + [NONE] * 4
    for s in range(64):
        assert ("b%d" % s in got.files) == (s < 60)
        if s < 60:
            assert got["b%d" % s].tolist() == sorted(B[s]), s


@pytest.mark.parametrize("n", [4096, 8192])
def test_shipped_ring_sizes_paterson_stockmeyer_layout(n):
    """the two transform forms the persistent kernel has besides the toy's: an 18-bit plain modulus (a few dozen cosets), about 100
    occupied bins spread over the slot range, counts up to 40 with double roots; degree 40 > ps_low_degree takes the
    Paterson-Stockmeyer layout"""
    js = common.toy_json(n=n, plain_bits=18, max_items=45)
    t = U.toy_t(js)
    assert (t - 1) // n < 64
    rng = np.random.default_rng(n)
    G = apsu_amd.HeContext(js)
    nb = n - 3
    B = [[] for _ in range(nb)]
    slots = sorted(set([0, 1, 63, 64, nb - 1] + [int(v) for v in rng.integers(0, nb, 96)]))
    for i, s in enumerate(slots):
        c = 40 if i % 10 == 0 else int(rng.integers(1, 41))
        vals = U.distinct(rng, t, max(1, c - c // 4))
        B[s] = (vals + [vals[k % len(vals)] for k in range(c - len(vals))])[:c]      # every fourth item repeats an earlier one
    B[slots[1]] = [0, 0, 0, t - 1]
    b = G.build_bundle(0, 0, B)
    assert b.degree == 40
    got = check_bins(G, b, B, forms=(KERNEL, COMPOSED))
    assert got[nb:] == [None] * 3
    G.close()


def test_bins_after_merge_update_and_image_round_trip():
    js = common.toy_json()
    t = U.toy_t(js)
    rng = np.random.default_rng(62)
    G = apsu_amd.HeContext(js)
    A = U.rand_bins(rng, t, 60, 5)
    Bb = [U.distinct(rng, t, int(rng.integers(0, 6))) for _ in range(60)]          # values may meet A's: multiple roots
    Bb[2] = list(A[2])                                                               # every item of the bin twice
    a, b = G.build_bundle(0, 0, A), G.build_bundle(0, 1, Bb)
    merged = G.merge_bundles([a, b])
    union = [x + y for x, y in zip(A, Bb)]
    check_bins(G, merged, union)
    ins, rem = U.mixed_lists(rng, t, A, 10)
    up = G.update_bundle(a, inserts=ins, removes=rem)
    model = U.apply_update(A, ins, rem)
    check_bins(G, up, model)
    G2 = apsu_amd.HeContext(js)                                                      # a context that knows the image only
    loaded = G2.load_bundle(G.save_bundle(merged))
    assert as_lists(G2.bins(loaded)) == want_lists(union, G.n)
    G2.close()
    G.close()


def test_refusals_leave_the_bundle_usable():
    js = common.toy_json()
    t = U.toy_t(js)
    G = apsu_amd.HeContext(js)
    B = toy_bins(t)
    b = G.build_bundle(0, 0, B)
    lib = E.load_library()
    counts = np.zeros(G.n, dtype=np.uint32)
    roots = np.full((G.n, 9), 0xAB, dtype=np.uint64)                                # the largest count is 10
    with pytest.raises(ValueError, match="stride 9"):
        E._check(lib.apsu_he_bundle_bins(G.h, b.h, C.c_void_p(roots.ctypes.data), C.c_void_p(counts.ctypes.data), C.c_uint32(9)))
    assert (roots == 0xAB).all()                                                    # nothing is written past the counts
    assert [int(c) for c in counts[:60]] == [len(x) for x in B]
    E._check(lib.apsu_he_bundle_bins(G.h, b.h, None, C.c_void_p(counts.ctypes.data), C.c_uint32(0)))      # counts alone
    assert [int(c) for c in counts] == [len(x) for x in B] + [NONE] * 4
    entry = (1, [B[1 + j][0] for j in range(5)])                                    # start bin 1: part j is an item of bin 1 + j
    assert G.lookup([b], [entry])[0][0][0]
    # a polynomial that is no product of linear factors: random coefficients
    r = G.random_bundle(0, 1, 7, 1234)
    roots = np.full((G.n, 7), 0xAB, dtype=np.uint64)
    with pytest.raises(ValueError, match=r"bin \d+: .*degree 7 does not split") as ei:
        E._check(lib.apsu_he_bundle_bins(G.h, r.h, C.c_void_p(roots.ctypes.data), C.c_void_p(counts.ctypes.data), C.c_uint32(7)))
    assert (roots == 0xAB).all() and (counts == 7).all()
    assert "roots found" in str(ei.value)
    with pytest.raises(ValueError, match="does not split"):
        G.bins(r, _form=COMPOSED)
    assert G.lookup([b], [entry])[0][0][0] and as_lists(G.bins(b)) == want_lists(B, G.n)
    G.close()
    # the 33-bit toy context of the merge test: 2^27 cosets
    js33 = common.toy_json(plain_bits=33, max_items=20, felts=3)
    t33 = U.toy_t(js33)
    G = apsu_amd.HeContext(js33)
    b = G.build_bundle(0, 0, [[1, 2, t33 - 1], [7]])
    with pytest.raises(E.ApsuHeError, match=str(t33) + r".*" + str((t33 - 1) // 64)):
        G.bins(b)
    assert not G.lookup([b], [(0, [1, 7, 0])])[0][0][0] and [int(c) for c in G.bin_counts(b)[:3]] == [3, 1, NONE]
    G.close()


def test_bins_through_the_multi_device_handle():
    js = common.toy_json()
    t = U.toy_t(js)
    rng = np.random.default_rng(63)
    G = apsu_amd.HeContext(js)
    parts = [toy_bins(t), U.rand_bins(rng, t, 60, 6)]
    M = apsu_amd.MultiContext(js, [0, 0])
    for slot, B in enumerate(parts):
        bid = M.build_bundle(slot, 0, B, slot=slot)
        assert M.bundle_info(bid)[0] == slot
        single = as_lists(G.bins(G.build_bundle(slot, 0, B)))
        assert as_lists(M.bins(bid)) == single == want_lists(B, G.n)
    with pytest.raises(ValueError):
        M.bins(2)                                                                    # no such id
    M.close()
    G.close()
