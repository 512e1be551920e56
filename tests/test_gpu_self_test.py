"""GPU tier of the plaintext check of a resident database: apsu_he_bundles_eval_plain (k_bins_eval behind Engine::decode_bundle),
apsu_he_db_self_test and apsu_he_multi_db_self_test.  Ground truths: Python-integer Horner evaluation of the bins' polynomials, and the
engine's own querier run through its separate calls (keygen .. decrypt_decode_budget) with the self-test's seed.  All comparisons are
exact: no tolerance enters anywhere.  Contexts: the toy set (n = 64: one wave, one tile) and a shipped set with n = 4096 and 4095 bins,
each with and without Paterson-Stockmeyer; all four have key switching (two or more coefficient primes), which the self-test needs."""
import numpy as np
import pytest
import torch

import apsu_amd
import common
import test_gpu_bundle_update as U
from oracle import ref
from test_gpu_query_side import params

pytestmark = pytest.mark.gpu

SEED = bytes((7 * i + 19) & 0xFF for i in range(64))
SEED_WORDS = np.frombuffer(SEED, dtype="<u8").astype(np.uint64)
X_FIRST, MASK_FIRST = 1 << 37, 1 << 38                    # bin_eval.h: where the self-test draws slot values and masks
# name -> (parameter set, bins per BinBundle, largest bin the test builds)
CASES = {"toy-ps": ("toy", 60, 7), "toy-plain": ("toy-nops", 60, 3), "n4096-ps": ("1M-1024-com", 4095, 9), "n4096-plain": ("256K-4096-cmp", 4095, 6)}


def poly_from_roots(roots, t):
    p = [1]
    for r in roots:
        q = [0] * (len(p) + 1)
        for i, c in enumerate(p):
            q[i + 1] = (q[i + 1] + c) % t
            q[i] = (q[i] - c * r) % t
        p = q
    return p


def horner(col, x, t):
    acc = 0
    for c in reversed(col):
        acc = (acc * x + c) % t
    return acc


def expected(bins, x, mask, t, n):
    """bins: per slot a list of roots (None or beyond the list: the zero polynomial)"""
    out = []
    for s in range(n):
        b = bins[s] if s < len(bins) else None
        v = 0 if b is None else horner(poly_from_roots(b, t), int(x[s]), t)
        out.append((v + (int(mask[s]) if mask is not None else 0)) % t)
    return np.array(out, dtype=np.uint64)


class Db:
    """one context with two healthy BinBundles per case, one per bundle index where the set has two, and the querier's separate calls
    run once with the self-test's seed and draws"""

    def __init__(self, case):
        name, self.n_bins, self.max_count = CASES[case]
        self.js = params(name)
        self.G = G = apsu_amd.HeContext(self.js)
        self.t, self.n = G.t, G.n
        rng = np.random.default_rng(len(case))
        self.idx = [0, 1] if G.bundle_idx_count >= 2 else [0, 0]
        self.bins = [U.rand_bins(rng, self.t, self.n_bins, self.max_count) for _ in range(2)]
        for b in self.bins:
            b[3] = []                                     # an empty bin: the polynomial 1
            b[7] = [0] + b[7][:2]                         # the root 0
        self.gb = [G.build_bundle(self.idx[i], i, self.bins[i]) for i in range(2)]
        self.loop = None

    def separate_calls(self):
        """what the self-test strings together, call by call: -> (x [distinct idx][n], mask values [2][n], decrypted [2][n], budgets [2])"""
        if self.loop is None:
            G, n = self.G, self.n
            didx = sorted(set(self.idx))
            L, S = G.first_chain_idx + 1, G.source_power_count
            scratch = torch.empty(len(didx) * n, dtype=torch.int64, device="cuda")
            x, _ = G.mask_generate_blake2xb(SEED_WORDS, len(didx), scratch.data_ptr(), first_value=X_FIRST, want_blocks=False)
            mbuf = torch.empty(2 * n, dtype=torch.int64, device="cuda")
            mask_vals, _ = G.mask_generate_blake2xb(SEED_WORDS, 2, mbuf.data_ptr(), first_value=MASK_FIRST, want_blocks=False)
            sk = G.keygen(SEED)
            _, _, rk = G.relin_keygen(sk, SEED, want_host=False)
            dev = torch.zeros((len(didx) * S, 2, L, n), dtype=torch.int64, device="cuda")
            G.query_create(sk, didx, np.ascontiguousarray(x), dev.data_ptr(), seed=SEED)
            ptrs = [[dev.data_ptr() + ((b * S + s) * 2 * L * n) * 8 for s in range(S)] for b in range(len(didx))]
            pw = G.compute_powers(didx, ptrs, rk, on_device=True)
            out = torch.empty((2, 2, n), dtype=torch.int64, device="cuda")
            G.eval_bundles(self.gb, pw, rk, [mbuf.data_ptr() + i * n * 8 for i in range(2)], out=out.data_ptr(), masks_on_device=True, out_on_device=True)
            got, _, bits = G.decrypt_decode(sk[0], out.data_ptr(), count=2, on_device=True, want_blocks=False, want_budget=True)
            self.loop = (x.reshape(len(didx), n), mask_vals.reshape(2, n), got.reshape(2, n), [int(b) for b in bits])
        return self.loop

    def x_rows(self, x):
        didx = sorted(set(self.idx))
        return np.stack([x[didx.index(i)] for i in self.idx])


@pytest.fixture(scope="module", params=list(CASES))
def db(request):
    d = Db(request.param)
    yield d
    d.G.close()


# ---- 1: eval_plain against Python Horner
def query_values(rng, bins, t, n):
    """random values; every third slot asks for one of its bin's items where it has any"""
    x = rng.integers(0, t, n, dtype=np.uint64)
    for s in range(0, len(bins), 3):
        if bins[s]:
            x[s] = bins[s][s % len(bins[s])]
    return x


def check_eval(G, gb, bins, rng, t, n):
    x = query_values(rng, bins, t, n)
    mask = rng.integers(0, t, n, dtype=np.uint64)
    out, is_bin = G.eval_plain([gb], x[None], want_is_bin=True)
    assert (out[0] == expected(bins, x, None, t, n)).all()
    assert [bool(v) for v in is_bin[0]] == [s < len(bins) and bins[s] is not None for s in range(n)]
    masked = G.eval_plain([gb], x[None], masks=mask[None])[0]
    assert (masked == expected(bins, x, mask, t, n)).all()
    member = np.array([s >= len(bins) or int(x[s]) in bins[s] for s in range(n)])
    assert member[len(bins):].all() and member[:len(bins)].any() and not member.all()
    assert (masked[member] == mask[member]).all() and (out[0][member] == 0).all()


def test_eval_plain_equals_python_horner(db):
    G, t, n = db.G, db.t, db.n
    rng = np.random.default_rng(5)
    for gb, bins in zip(db.gb, db.bins):
        check_eval(G, gb, bins, rng, t, n)
    # both BinBundles in one call, each with its own row
    x = np.stack([query_values(rng, b, t, n) for b in db.bins])
    mask = rng.integers(0, t, (2, n), dtype=np.uint64)
    out = G.eval_plain(db.gb, x, masks=mask)
    for i in range(2):
        assert (out[i] == expected(db.bins[i], x[i], mask[i], t, n)).all()
    # points 0, 1 and t - 1 everywhere
    for v in (0, 1, t - 1):
        xs = np.full(n, v, dtype=np.uint64)
        assert (G.eval_plain([db.gb[0]], xs[None])[0] == expected(db.bins[0], xs, None, t, n)).all()


def test_eval_plain_follows_update_merge_and_image(db):
    G, t, n = db.G, db.t, db.n
    rng = np.random.default_rng(6)
    bins = [list(b) for b in db.bins[0]]
    # update: an insertion into the empty bin and into a full one's neighbour, a removal
    ins, rem = [[] for _ in bins], [[] for _ in bins]
    ins[3] = U.distinct(rng, t, 2)
    rem[7] = [0]
    ins[9] = U.distinct(rng, t, 1, avoid=bins[9])
    up = G.update_bundle(db.gb[0], ins, rem)
    after = [sorted(set(b) - set(rem[s])) + ins[s] for s, b in enumerate(bins)]
    check_eval(G, up, after, rng, t, n)
    # merge with a sparse BinBundle of the same bundle index
    other = [U.distinct(rng, t, 1, avoid=after[s]) if s % 5 == 0 else [] for s in range(len(bins))]
    gb2 = G.build_bundle(db.idx[0], 7, other)
    merged = G.merge_bundles([up, gb2], cache_idx=0)
    union = [a + b for a, b in zip(after, other)]
    check_eval(G, merged, union, rng, t, n)
    # image round trip
    check_eval(G, G.load_bundle(G.save_bundle(merged)), union, rng, t, n)


# ---- 2: decrypt(eval(query)) = eval_plain, slot for slot
def test_decrypted_evaluation_equals_eval_plain(db):
    x, mask_vals, got, bits = db.separate_calls()
    want = db.G.eval_plain(db.gb, db.x_rows(x), masks=mask_vals)
    print("noise budgets:", bits)
    assert min(bits) > 0
    assert (got == want).all()
    for i in range(2):
        assert (want[i] == expected(db.bins[i], db.x_rows(x)[i], mask_vals[i], db.t, db.n)).all()


# ---- 3: the self-test on a healthy database
def test_self_test_on_a_healthy_database(db):
    x, mask_vals, got, bits = db.separate_calls()
    rep = db.G.self_test(db.gb, SEED)
    print(rep)
    assert (rep.bundles, rep.slots, rep.mismatches, rep.first_mismatch) == (2, 2 * db.n, 0, None)
    assert rep.min_budget == min(bits) and rep.min_budget_bundle == bits.index(min(bits))
    assert rep.he_ms > 0 and rep.plain_ms > 0
    # slot values given by the caller: the bins' own items decrypt to the masks alone, and the test still passes
    xs = np.stack([query_values(np.random.default_rng(8), db.bins[db.idx.index(i)], db.t, db.n) for i in sorted(set(db.idx))])
    rep = db.G.self_test(db.gb, SEED, x=xs)
    assert (rep.bundles, rep.mismatches, rep.first_mismatch) == (2, 0, None)
    # the context still answers queries after its workspace was cleared
    assert (db.G.eval_plain(db.gb, db.x_rows(x), masks=mask_vals) == got).all()
    assert db.G.self_test([], SEED) == apsu_amd.engine.SelfTestReport(0, 0, 0, None, 0, None, 0.0, 0.0)


# ---- 4: the self-test has teeth
def damaged_coeffs(js, bins, ps_low):
    """the stored coefficients of build_bundle(bins) with ONE word of one NTT-form degree changed: its limbs no longer describe one
    plaintext, so the evaluation and the decoded polynomial part ways (a change that is itself a valid plaintext -- a_0, or a
    coefficient-form a_{ih} -- would be another database, which no self-test can tell from the intended one)"""
    C = ref.RefContext.from_params(ref.load_params(js))
    _, coeffs, flags = U.oracle_build(C, ps_low, bins)
    d = max(i for i, f in enumerate(flags) if f)
    bad = [np.array(c, dtype=np.uint64, copy=True) for c in coeffs]
    flat = bad[d].reshape(-1)
    flat[11] = (int(flat[11]) + 1) % C.q[0]
    return coeffs, bad, flags, d


def test_self_test_names_a_damaged_bundle():
    js = common.toy_json()
    G = apsu_amd.HeContext(js)
    t = G.t
    rng = np.random.default_rng(9)
    bins = U.rand_bins(rng, t, 60, 10)
    good = G.build_bundle(0, 0, bins)
    coeffs, bad, flags, d = damaged_coeffs(js, bins, G.ps_low_degree)
    same = G.upload_bundle(0, 1, coeffs, flags)
    hurt = G.upload_bundle(0, 2, bad, flags)
    assert G.self_test([good, same], SEED).mismatches == 0                     # the upload itself is healthy
    rep = G.self_test([good, hurt], SEED)
    print(rep)
    assert rep.mismatches > 0 and rep.first_mismatch[0] == 1 and rep.first_mismatch[2] != rep.first_mismatch[3]
    rep = G.self_test([hurt, good], SEED)
    assert rep.mismatches > 0 and rep.first_mismatch[0] == 0
    assert G.self_test([good], SEED).mismatches == 0                           # the healthy neighbour alone
    G.close()


# ---- 5: the multi-device handle, on a device list that repeats one GPU
@pytest.mark.parametrize("devs", [[0], [0, 0], [0, 0, 0]], ids=lambda d: "devs" + "".join(str(x) for x in d))
def test_multi_self_test_equals_the_single_context(devs):
    js = common.toy_json()
    G = apsu_amd.HeContext(js)
    M = apsu_amd.MultiContext(js, devs)
    t = G.t
    rng = np.random.default_rng(10)
    assert M.self_test(SEED)[:4] == (0, 0, 0, None)                            # an empty handle
    single = []
    for k, (bidx, cidx) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)]):
        bins = U.rand_bins(rng, t, 60, 4 + 2 * k)
        assert M.build_bundle(bidx, cidx, bins, slot=k % len(devs)) == k
        single.append(G.build_bundle(bidx, cidx, bins))
    a, b = M.self_test(SEED), G.self_test(single, SEED)
    print(a, b)
    assert a[:6] == b[:6] and a.mismatches == 0 and a.bundles == 4
    # a damaged BinBundle is named by its id
    bins = U.rand_bins(rng, t, 60, 10)
    _, bad, flags, _ = damaged_coeffs(js, bins, G.ps_low_degree)
    assert M.upload_bundle(len(devs) - 1, 0, 2, bad, flags) == 4
    single.append(G.upload_bundle(0, 2, bad, flags))
    a, b = M.self_test(SEED), G.self_test(single, SEED)
    assert a[:6] == b[:6] and a.mismatches > 0 and a.first_mismatch[0] == 4
    M.close()
    G.close()


# ---- 6: refusals
def test_refusals():
    G = apsu_amd.HeContext(common.toy_json())
    t, n = G.t, G.n
    gb = G.build_bundle(0, 0, U.rand_bins(np.random.default_rng(11), t, 60, 4))
    x = np.zeros((1, n), dtype=np.uint64)
    bad = x.copy()
    bad[0, 63] = t
    with pytest.raises(ValueError):
        G.eval_plain([gb], bad)
    with pytest.raises(ValueError):
        G.eval_plain([gb], x, masks=bad)
    with pytest.raises(ValueError):
        G.self_test([gb], SEED, x=bad)
    # the same value met on the device
    lib = apsu_amd.engine.load_library()
    import ctypes as C
    hs = (C.c_void_p * 1)(gb.h)
    xd = torch.from_numpy(bad.view(np.int64)).cuda()
    od = torch.zeros(n, dtype=torch.int64, device="cuda")
    assert lib.apsu_he_bundles_eval_plain(G.h, hs, 1, C.c_void_p(xd.data_ptr()), 1, None, 0, C.c_void_p(od.data_ptr()), 1, None) == -1
    good = torch.from_numpy(x.view(np.int64)).cuda()
    assert lib.apsu_he_bundles_eval_plain(G.h, hs, 1, C.c_void_p(good.data_ptr()), 1, None, 0, C.c_void_p(od.data_ptr()), 1, None) == 0
    assert (od.cpu().numpy().view(np.uint64) == G.eval_plain([gb], x)[0]).all()
    G.close()
    # no PSUParams, with and without a batching plain modulus (PSUParams themselves demand batching): a logic error, as from
    # apsu_he_bundle_bin_counts
    C_ = ref.RefContext.from_params(ref.load_params(common.toy_json()))
    for plain in (C_.t, 65539):                                                # 65539 is prime and 3 mod 128
        raw = apsu_amd.HeContext(n=64, coeff_modulus=C_.q, plain_modulus=plain)
        with pytest.raises(apsu_amd.engine.ApsuHeError):
            raw.self_test([], SEED)
        hs0 = (C.c_void_p * 1)()
        assert lib.apsu_he_bundles_eval_plain(raw.h, hs0, 0, None, 0, None, 0, None, 0, None) == -2
        raw.close()
    # one coefficient prime: no key switching.  eval_plain serves the set, the self-test refuses it as relin_keygen does
    one = apsu_amd.HeContext(params("single-prime"))
    assert one.K == 1 and one.t % (2 * one.n) == 1
    b1 = one.build_bundle(0, 0, [[1, 2], [3]])
    xs = np.full((1, one.n), 2, dtype=np.uint64)
    assert (one.eval_plain([b1], xs)[0] == expected([[1, 2], [3]], xs[0], None, one.t, one.n)).all()
    with pytest.raises(ValueError, match="key switching"):
        one.self_test([b1], SEED)
    one.close()
