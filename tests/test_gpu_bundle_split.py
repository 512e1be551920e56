"""GPU tier: apsu_he_bundle_split -- one resident BinBundle cut into k parts on the device (k_roots_split behind the root search, then the
tail of the build per part), and the ROOTS_SPLIT step, which puts chosen lists in front of that one kernel.  The contract is the
build's: the image of part p of split(build(B), k) is byte-identical to that of build_bundle of part p of B under
split_cut(c, k, p) = p c // k (tests/split_model.py: sorted() and slicing), and merging the parts gives the input's image back."""
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


def check_split(G, bins, k, built=None, bundle_idx=0, cache_idx=3, part_cache=None, merge_back=True):
    """split(build(bins), k) against build_bundle of the model's parts -> the parts"""
    b = built or G.build_bundle(bundle_idx, cache_idx, bins)
    before = image(G, b)
    parts = G.split_bundle(b, k, cache_idx=part_cache)
    assert len(parts) == k
    want = M.split_bins(bins, k)
    for p, part in enumerate(parts):
        ci = b.cache_idx + p if part_cache is None else part_cache[p]
        assert (part.bundle_idx, part.cache_idx) == (b.bundle_idx, ci)
        rebuilt = G.build_bundle(b.bundle_idx, ci, want[p])
        assert part.degree == rebuilt.degree == max(len(x) for x in want[p])
        assert image(G, part) == image(G, rebuilt), "part %d of %d: image differs from build_bundle of the model's part" % (p, k)
        counts = G.bin_counts(part)
        assert [int(c) for c in counts[:len(bins)]] == [len(x) for x in want[p]] and (counts[len(bins):] == NONE).all()
    assert image(G, b) == before                            # the input is only read
    if merge_back and k >= 2:
        assert image(G, G.merge_bundles(parts, cache_idx=b.cache_idx)) == before
    return parts


def toy_bins(rng, t, n_bins=60, most=10):
    bins = U.rand_bins(rng, t, n_bins, most - 1, full_frac=0.1)
    bins[0] = U.distinct(rng, t, most)                     # the largest count
    bins[3] = []                                           # count 0
    bins[4] = U.distinct(rng, t, 1)                        # count 1
    bins[7] = [0]                                          # the root 0 alone
    bins[9] = [0] + U.distinct(rng, t, 6)
    return bins


@pytest.mark.parametrize("k", [1, 2, 3, 10])
def test_split_images_equal_the_build_of_the_models_parts(k):
    js = common.toy_json()
    t = U.toy_t(js)
    rng = np.random.default_rng([51, k])
    G = apsu_amd.HeContext(js)
    bins = toy_bins(rng, t)
    bins[5] = U.distinct(rng, t, max(k - 1, 0))            # count k - 1: empty in one part
    check_split(G, bins, k, part_cache=None if k != 3 else [9, 4, 20])
    ms = G.split_times()
    assert len(ms) == 4 and all(m >= 0 for m in ms) and ms[1] > 0
    G.close()


def test_split_multiple_roots_straddle_the_cuts():
    js = common.toy_json()
    t = U.toy_t(js)
    rng = np.random.default_rng(52)
    G = apsu_amd.HeContext(js)
    bins = [[] for _ in range(60)]
    bins[0] = [5, 5, 9, 9, 9, 12]                          # k = 2 cuts at 3 (inside the triple 9), k = 3 at 2 and 4
    bins[1] = [0, 0, 0, 7]                                 # the root 0, three times
    bins[2] = [t - 1] * 6                                  # one root of multiplicity c
    bins[30] = sorted(U.distinct(rng, t, 4) * 2)           # four double roots
    bins[59] = [3, 3]
    for k in (2, 3, 6):
        check_split(G, bins, k)
    G.close()


def test_split_after_update_merge_and_image_round_trip():
    js = common.toy_json()
    t = U.toy_t(js)
    rng = np.random.default_rng(53)
    G = apsu_amd.HeContext(js)
    A = U.rand_bins(rng, t, 60, 4, full_frac=0.2)
    B = [U.distinct(rng, t, int(rng.integers(0, 4)), avoid=a) for a in A]
    B[6] = list(A[6][:1]) + B[6][:2]                       # a double root made by the merge
    a, b = G.build_bundle(1, 0, A), G.build_bundle(1, 1, B)
    merged = G.merge_bundles([a, b])
    bins = [x + y for x, y in zip(A, B)]
    check_split(G, bins, 2, built=merged)
    ins = [U.distinct(rng, t, 1, avoid=x) if s % 3 == 0 else [] for s, x in enumerate(bins)]
    rem = [[x[0]] if s % 3 == 1 and x else [] for s, x in enumerate(bins)]
    up = G.update_bundle(merged, inserts=ins, removes=rem)
    bins2 = U.apply_update(bins, ins, rem)
    check_split(G, bins2, 3, built=up)
    loaded = G.load_bundle(G.save_bundle(up))              # a BinBundle whose roots this context never saw
    loaded.bundle_idx, loaded.cache_idx = up.bundle_idx, up.cache_idx      # (the wrapper of a loaded image does not know them; the engine does)
    check_split(G, bins2, 2, built=loaded)
    G.close()


def test_split_of_a_paterson_stockmeyer_bundle_into_parts_below_ps_low_degree():
    # toy ps_low_degree = 3: degree 9 has the Paterson-Stockmeyer layout, its three parts of degree 3 are all NTT-form
    js = common.toy_json()
    t = U.toy_t(js)
    rng = np.random.default_rng(54)
    G = apsu_amd.HeContext(js)
    bins = U.rand_bins(rng, t, 60, 9, full_frac=0.3)
    bins[2] = U.distinct(rng, t, 9)
    b = G.build_bundle(0, 0, bins)
    parts = check_split(G, bins, 3, built=b)
    assert b.degree == 9 and [p.degree for p in parts] == [3, 3, 3]
    G.close()


def test_split_four_tiles_composed_search_and_a_slot_that_is_not_a_bin():
    js = common.toy_json(n=256)                             # no persistent kernel at this ring size: the per-coset composition
    t = U.toy_t(js)
    rng = np.random.default_rng(55)
    G = apsu_amd.HeContext(js)
    bins = U.rand_bins(rng, t, 255, 6, full_frac=0.1)       # slot 255 holds the zero polynomial
    bins[254] = U.distinct(rng, t, 10)
    bins[64] = [0, 0, 1]
    check_split(G, bins, 3)
    G.close()


@pytest.mark.parametrize("name,most", [("1M-512-com", 227), ("256K-2048-cmp", 31)])
def test_split_shipped_parameters(name, most):
    js = common.param_json(name)
    G = apsu_amd.HeContext(js)
    assert G.n == 4096 and G.t == 65537
    rng = np.random.default_rng([56, most])
    bins = [[] for _ in range(40)]
    for s in range(0, 40, 2):                               # twenty occupied bins
        bins[s] = U.distinct(rng, G.t, int(rng.integers(1, most // 2)))
    bins[6] = U.distinct(rng, G.t, most)
    bins[8] = [0] + sorted(U.distinct(rng, G.t, most // 4) * 2)
    check_split(G, bins, 2, merge_back=False)               # (a bin at the bound cannot be merged back: the merge's own refusal)
    G.close()


def test_split_refusals_leave_the_context_working():
    js = common.toy_json()
    t = U.toy_t(js)
    rng = np.random.default_rng(57)
    G = apsu_amd.HeContext(js)
    bins = toy_bins(rng, t)
    b = G.build_bundle(0, 0, bins)
    with pytest.raises(ValueError, match="1 part or more"):
        G.split_bundle(b, 0)
    with pytest.raises(ValueError, match="11 parts, but the largest bin holds 10 items"):
        G.split_bundle(b, 11)
    check_split(G, bins, 2, built=b)
    r = G.random_bundle(0, 1, 6, 99)                        # random polynomials: (almost) none is a product of linear factors
    with pytest.raises(ValueError, match=r"bin \d+: its polynomial of degree 6 does not split into linear factors \(\d+ roots found"):
        G.split_bundle(r, 2)
    check_split(G, bins, 3, built=b)                        # the context goes on after every refusal
    empty = G.build_bundle(0, 5, [[] for _ in range(60)])   # no occupied bin: any k, every part empty
    parts = G.split_bundle(empty, 4)
    assert [p.degree for p in parts] == [0] * 4 and all(image(G, p)[256:] == image(G, empty)[256:] for p in parts)
    G.close()


# --------------------------------------------------------------------------------------------- the step entry: k_roots_split alone
def run_step(G, case):
    hits, found, mult, occ = case.inputs()
    out = np.full(case.off[-1], M.POISON, dtype=np.uint64)
    tail = np.full(case.k * case.n + 1, 0x77, dtype=np.uint64)
    u64 = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
    G.debug_run_step("roots_split", 0, ins=[u64(hits), u64(found), u64(mult), u64(case.counts), u64(case.stride)], outs=[out, tail], polys=case.k,
                     e0=case.hstride, batch=0)
    return out, tail[:-1].reshape(case.k, case.n).astype(np.uint32), int(tail[-1])


def check_case(got, case):
    want_out, want_counts, want_failure = case.expected()
    out, counts_out, failure = got
    assert failure == want_failure, case.name
    assert (counts_out == want_counts).all(), case.name
    bad = np.flatnonzero(out != want_out)
    assert not len(bad), "%s: %d words differ, first at %d: got %#x, want %#x" % (case.name, len(bad), bad[0], int(out[bad[0]]), int(want_out[bad[0]]))


def test_roots_split_step_adversarial_lists_and_every_instance():
    js = common.toy_json()
    G = apsu_amd.HeContext(js)
    cases = M.adversarial_cases(G.t, G.n) + M.boundary_cases(G.t, G.n)
    assert {256, 2048, 8192} == {min(c for c in M.CAPS if case.hstride <= c) for case in cases}
    for case in cases:
        check_case(run_step(G, case), case)
    G.close()


def test_roots_split_step_refuses_what_lies_beyond_the_contract():
    js = common.toy_json()
    G = apsu_amd.HeContext(js)
    n, t = G.n, G.t
    good = M.Case("good", n, 8, 2, [M.Bin(3, [5, 9], mult=[2, 1], count=3)])
    check_case(run_step(G, good), good)

    def call(value=5, mult=2, stride=(2, 3), k=2, h=8):
        hits, mults = np.zeros((1, h), dtype=np.uint64), np.zeros((1, h), dtype=np.uint64)
        hits[0, :2], mults[0, :2] = [value, 9], [mult, 1]
        counts = np.full(n, NONE, dtype=np.uint64)
        counts[3] = 3
        words = n * sum(stride)
        G.debug_run_step("roots_split", 0, ins=[hits, np.array([2], dtype=np.uint64), mults, counts, np.array(stride, dtype=np.uint64)],
                         outs=[np.zeros(words, dtype=np.uint64), np.zeros(max(k, 1) * n + 1, dtype=np.uint64)], polys=k, e0=h, batch=0)

    call()
    for what, kw in ((r"k \(polys\) out of range", dict(k=0)), ("no instance holds the list", dict(h=8193)), ("a count exceeds hstride", dict(h=2)),
                     ("is not below min", dict(value=t)), ("exceeds SPLIT_MULT_MAX", dict(mult=(1 << 18) + 1)), ("part_stride is below", dict(stride=(1, 1))),
                     ("wrong size", dict(stride=(2, 3, 1)))):
        with pytest.raises(ValueError, match=what):
            call(**kw)
    check_case(run_step(G, good), good)                      # the context goes on
    G.close()
