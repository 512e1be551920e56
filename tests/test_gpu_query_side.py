"""GPU tier -- N5, the querier's side on the device: key generation, relinearisation keys, query encryption and the invariant noise
budget (apsu_he_keygen / _relin_keygen / _query_create / _decrypt_decode_budget).  The oracle is the checker here, never the
producer: the engine's outputs are taken apart with the oracle's transforms and compared with the Python model of the documented
random streams (query_side_model.py), then the loop keygen -> query -> ComputePowers -> eval -> decrypt runs on nothing but the
engine and is compared bit for bit with the oracle fed the same GPU-made inputs."""
import json

import numpy as np
import pytest

import apsu_amd
import common
import query_side_model as M
from apsu_amd import seal, wire
from oracle import ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED = bytes((11 * i + 3) & 0xFF for i in range(64))
SEED2 = bytes((5 * i + 77) & 0xFF for i in range(64))


def params(name):
    if name == "toy":
        return common.toy_json()
    if name == "toy-nops":
        return common.toy_json(ps_low=0, max_items=6, query_powers=(1, 2, 3, 5))
    if name == "n32768":
        return common.toy_json(n=32768, coeff_bits=(56, 56, 56, 50), plain_bits=20, ps_low=2, max_items=8, query_powers=(1, 3), felts=5)
    if name == "n1024-60":
        return common.toy_json(n=1024, coeff_bits=(60, 60, 60, 50), plain_bits=17)
    if name == "single-prime":
        return common.toy_json(n=64, coeff_bits=(60,), plain_bits=9, felts=10, ps_low=0, max_items=4)
    return common.param_json(name)


KS_SETS = ["toy", "1M-1024-com", "16M-4096", "256M-4096", "n32768"]


class Side:
    """one parameter set: engine context, oracle context, and the oracle's transforms over ALL K key limbs"""

    def __init__(self, name):
        self.js = params(name)
        self.p = ref.load_params(self.js)
        self.C = ref.RefContext.from_params(self.p)
        self.G = apsu_amd.HeContext(self.js)
        C = self.C
        self.n, self.K, self.first, self.L, self.t = C.n, C.K, C.first, C.first + 1, C.t
        self.sources = sorted(self.p["query_powers"])
        self.S = len(self.sources)
        # the special prime's transform: a context whose first (and only data) limb is that prime
        self.Cp = ref.RefContext(C.n, coeff_modulus=[C.q[C.K - 1], C.q[0]], plain_modulus=C.t) if C.K > 1 else None

    def intt(self, a):
        """[K or L][n] NTT form -> coefficient form, every limb with its own prime"""
        a = np.ascontiguousarray(a, dtype=np.uint64).copy()
        lo = np.ascontiguousarray(a[None, :self.L])
        self.C.transform_from_ntt(lo, self.first)
        out = [lo[0]]
        if a.shape[0] > self.L:
            hi = np.ascontiguousarray(a[None, self.L:self.L + 1])
            self.Cp.transform_from_ntt(hi, 0)
            out.append(hi[0])
        return np.concatenate(out)

    def c1_times_s(self, c1, sk):
        """[L][n] coefficient form x secret (NTT form) -> coefficient form"""
        v = np.ascontiguousarray(c1[None].copy())
        self.C.transform_to_ntt(v, self.first)
        v = self.C.multiply_plain_ntt(v, np.ascontiguousarray(sk[:self.L]), self.first)
        self.C.transform_from_ntt(v, self.first)
        return v[0]

    def delta(self, pt):
        d = np.zeros((2, self.L, self.n), dtype=np.uint64)
        self.C.add_plain(d, pt, self.first)
        return d[0]

    def slot_values(self, nb, seed=1):
        return np.random.default_rng(seed).integers(0, self.t, (nb, self.n), dtype=np.uint64)

    def query(self, sk, idx, values, seed=SEED, on_device=False):
        """-> (cts [count][2][L][n] host copy, seeds, device tensor)"""
        dev = torch.zeros((len(idx) * self.S, 2, self.L, self.n), dtype=torch.int64, device="cuda")
        if on_device:
            vd = torch.from_numpy(np.ascontiguousarray(values).view(np.int64)).cuda()
            seeds = self.G.query_create(sk, idx, vd.data_ptr(), dev.data_ptr(), seed=seed, values_on_device=True)
        else:
            seeds = self.G.query_create(sk, idx, values, dev.data_ptr(), seed=seed)
        torch.cuda.synchronize()
        return dev.cpu().numpy().view(np.uint64), seeds, dev

    def close(self):
        self.G.close()


def signed(r, q):
    """residues (uint64, < q) -> centred int64"""
    r = r.astype(np.int64)
    return np.where(r > q // 2, r - q, r)


def noise_of(sd, ct, sk, pt):
    """Delta(m) - c0 - c1 s per limb, centred: [L][n] int64"""
    v, d = sd.c1_times_s(ct[1], sk), sd.delta(pt)
    out = []
    for j in range(sd.L):
        q = np.uint64(sd.C.q[j])
        assert (ct[:, j] < q).all()
        out.append(signed((d[j] + q + q - ct[0, j] - v[j]) % q, int(q)))
    return np.stack(out)


def plain_of(sd, x, e):
    return sd.C.encode(np.array([pow(int(v), e, sd.t) for v in x], dtype=np.uint64))


# ---- 1: the key
@pytest.mark.parametrize("name", KS_SETS + ["single-prime"])
def test_secret_key(name):
    sd = Side(name)
    sk = sd.G.keygen(SEED)
    assert sk.shape == (sd.K, sd.n)
    for j in range(sd.K):
        assert (sk[j] < np.uint64(sd.C.q[j])).all()
    s = sd.intt(sk)
    model = M.secret(SEED, sd.n)
    for j in range(sd.K):
        sj = signed(s[j], sd.C.q[j])
        assert set(np.unique(sj)) <= {-1, 0, 1}
        assert (sj == model).all(), j
    if sd.n == 8192:
        sigma = (2 * sd.n / 9) ** 0.5
        for v in (-1, 0, 1):
            assert abs(int((model == v).sum()) - sd.n / 3) < 5 * sigma
    assert (sd.G.keygen(SEED) == sk).all() and (sd.G.keygen(SEED2) != sk).any()
    sd.close()


# ---- 2 + 3: the encryption is exact, and the oracle agrees on its meaning
@pytest.mark.parametrize("name", KS_SETS + ["single-prime"])
def test_query_encryption(name):
    sd = Side(name)
    C, G = sd.C, sd.G
    sk = G.keygen(SEED)
    bic = sd.p["bundle_idx_count"]
    idx = list(range(bic)) if name == "16M-4096" else list(range(min(bic, 2)))[::-1]
    x = sd.slot_values(len(idx))
    x[0, :3] = [0, 1, sd.t - 1]
    cts, seeds, _ = sd.query(sk, idx, x)
    count = len(idx) * sd.S
    assert cts.shape[0] == count and seeds.shape == (count, 8)
    sc = seal.SealContext(sd.js)
    all_noise, budgets, ref_budgets = [], [], []
    for c in range(count):
        b, e = c // sd.S, sd.sources[c % sd.S]
        pt = plain_of(sd, x[b], e)
        assert (seeds[c] == M.public_seed(SEED, M.KEY_OBJECTS + c)).all()
        assert (cts[c, 1] == sc.sample_poly_uniform(sd.first, [int(w) for w in seeds[c]], sd.L, sd.n)).all()
        en = noise_of(sd, cts[c], sk, pt)
        for j in range(1, sd.L):
            assert (en[j] == en[0]).all()                       # the same integer in every limb
        assert np.abs(en[0]).max() <= 21
        assert (en[0] == M.noise(SEED, M.KEY_OBJECTS + c, sd.n)).all(), c
        all_noise.append(en[0])
        got, budget = C.decrypt(sk, np.ascontiguousarray(cts[c]), sd.first)
        assert (got == pt).all()                                # 3: the oracle decrypts encode(x^e)
        budgets.append(budget)
        ref_budgets.append(C.decrypt(sk, C.encrypt(sk, pt, 4000 + c), sd.first)[1])
    print("fresh noise budget %s: engine min %d bits, oracle's encrypt min %d bits" % (name, min(budgets), min(ref_budgets)))
    assert min(budgets) >= min(ref_budgets) - 1
    assert len({s.tobytes() for s in seeds}) == count and len({a.tobytes() for a in all_noise}) == count
    if name == "16M-4096":
        e = np.concatenate(all_noise).astype(np.float64)
        N = e.size
        assert N >= 190000
        # a centred binomial over 21 coin pairs: variance 10.5, fourth central moment 3 * 10.5^2 - 10.5 / 2 = 325.5
        assert abs(e.mean()) < 5 * (10.5 / N) ** 0.5
        assert abs((e * e).mean() - 10.5) < 5 * ((325.5 - 10.5 ** 2) / N) ** 0.5
    # the same seed reproduces the query bit for bit (device-resident values take the same path), another seed changes every ciphertext
    again, seeds2, _ = sd.query(sk, idx, x, on_device=True)
    assert (again == cts).all() and (seeds2 == seeds).all()
    other, seeds3, _ = sd.query(sk, idx, x, seed=SEED2)
    for c in range(count):
        assert (other[c, 0] != cts[c, 0]).any() and (other[c, 1] != cts[c, 1]).any() and (seeds3[c] != seeds[c]).any()
    sd.close()


# ---- 4: relinearisation keys
@pytest.mark.parametrize("name", KS_SETS)
def test_relin_keys(name):
    sd = Side(name)
    C, G = sd.C, sd.G
    K, n = sd.K, sd.n
    sk = G.keygen(SEED)
    ksk, kseeds, resident = G.relin_keygen(sk, SEED)
    assert ksk.shape == (K - 1, 2, K, n) and kseeds.shape == (K - 1, 8)
    sc = seal.SealContext(sd.js)
    p = C.q[K - 1]
    for i in range(K - 1):
        assert (kseeds[i] == M.public_seed(SEED, i)).all()
        assert (ksk[i, 1] == sc.sample_poly_uniform(-1, [int(w) for w in kseeds[i]], K, n)).all()
        r = np.empty((K, n), dtype=np.uint64)
        for j in range(K):
            q = C.q[j]
            assert (ksk[i, :, j] < np.uint64(q)).all()
            s = sk[j].astype(object)
            v = ksk[i, 0, j].astype(object) + ksk[i, 1, j].astype(object) * s
            if j == i:
                v = v - (p % q) * s * s
            r[j] = (v % q).astype(np.uint64)
        e = sd.intt(r)                                          # = -e_i in every limb
        e0 = -signed(e[0], C.q[0])
        for j in range(K):
            assert (-signed(e[j], C.q[j]) == e0).all(), (i, j)
        assert np.abs(e0).max() <= 21 and (e0 == M.noise(SEED, i, n)).all()
    # the oracle multiplies and relinearises WITH THE ENGINE'S KEYS
    rng = np.random.default_rng(8)
    a, b = rng.integers(0, sd.t, (2, n), dtype=np.uint64)
    ca, cb = C.encrypt(sk, C.encode(a), 1), C.encrypt(sk, C.encode(b), 2)
    prod = C.relinearize(C.multiply(ca, cb, sd.first), ksk, sd.first)
    pt, budget = C.decrypt(sk, prod, sd.first)
    assert budget > 0 and (C.decode(pt).astype(object) == (a.astype(object) * b.astype(object)) % sd.t).all()
    # the resident handle and the uploaded host copy give the same ComputePowers bits
    targets = ref.create_powers_set(sd.p["ps_low_degree"], sd.p["max_items_per_bin"])
    cts, _, dev = sd.query(sk, [0], sd.slot_values(1))
    ptrs = [[dev.data_ptr() + s * 2 * sd.L * n * 8 for s in range(sd.S)]]
    pw1 = G.compute_powers([0], ptrs, resident, on_device=True)
    got1 = [pw1.download(0, t)[0].copy() for t in targets]
    pw2 = G.compute_powers([0], [[cts[s] for s in range(sd.S)]], G.upload_relin_keys(ksk))
    for t, g1 in zip(targets, got1):
        assert (pw2.download(0, t)[0] == g1).all(), t
    assert (G.relin_keygen(sk, SEED, want_resident=False)[0] == ksk).all()
    sd.close()


def test_seed_expansion_waiting_and_queued_agree_at_the_key_level(monkeypatch):
    """One set-up, two entries: relin_keygen queues the expansion of its public halves, apsu_he_seed_expand waits for its own.  At a
    key level above the first data level (K = 3 on the smallest ring) both read the engine's moduli-only view of that level; the same
    seeds must give the same words either way, and again in a fresh context that expands on the host (APSU_HE_SEED_EXPAND_HOST=1)."""
    js = common.toy_json(coeff_bits=(40, 40, 36))
    words = []
    for host in (False, True):
        if host:
            monkeypatch.setenv("APSU_HE_SEED_EXPAND_HOST", "1")
        G = apsu_amd.HeContext(js)
        K, n = G.K, 64
        assert K == 3 and K - 1 > G.first_chain_idx
        ksk, kseeds = G.relin_keygen(G.keygen(SEED), SEED, want_resident=False)[:2]
        out = torch.zeros((K - 1, K, n), dtype=torch.int64, device="cuda")
        for _ in range(2):                                      # (the second call finds the view uploaded)
            G.seed_expand(-1, kseeds, [out.data_ptr() + i * K * n * 8 for i in range(K - 1)])
            waited = out.cpu().numpy().view(np.uint64)
            assert (waited == ksk[:, 1]).all()
        words.append(waited)
        G.close()
    assert (words[0] == words[1]).all()


@pytest.mark.parametrize("which", ["cap 16", "median"])
def test_overflowing_seed_lists_give_the_words_of_a_context_without_the_switch(monkeypatch, which):
    """relin_keygen queues the expansion of its public halves and runs the rest of its work behind it; when an object has refused more
    words than its device list holds, the host redoes every object and the rest runs a second time.  Driven at a small size by
    APSU_HE_SEED_REJ_CAP with primes that refuse one word in 17 (query_step_model.high_rejection_primes): about 240 per key at
    n = 1024.  With a cap of 16 every key overflows, with the median of the keys' counts (the model's) one does.  Every word must be
    what a context without the switch returns, and the same call again must be exact too: the lists were left clean.

    query_create has the same fallback, but no context can take it: it needs a parameter file, a parameter file gives SEAL's primes
    2^b - c, and those refuse 2^(64 - b) c words in 2^64 -- the objects of the 60-bit set below refuse none, so there the switch must
    change nothing."""
    import query_step_model as QS
    n, t = 1024, 120833
    q = QS.high_rejection_primes(n, 4)
    plain = apsu_amd.HeContext(n=n, coeff_modulus=q, plain_modulus=t)
    sk = plain.keygen(SEED)
    ksk0, kseeds0 = plain.relin_keygen(sk, SEED, want_resident=False)[:2]
    plain.close()
    assert all((kseeds0[i] == M.public_seed(SEED, i)).all() for i in range(3))
    counts = [QS.rejection_count(sd, q, n) for sd in kseeds0]
    cap = 16 if which == "cap 16" else sorted(counts)[1]
    over = [c > cap for c in counts]
    assert min(counts) > 150 and any(over) and (which == "cap 16") == all(over), (counts, cap)
    monkeypatch.setenv("APSU_HE_SEED_REJ_CAP", str(cap))
    G = apsu_amd.HeContext(n=n, coeff_modulus=q, plain_modulus=t)
    assert (G.keygen(SEED) == sk).all()
    for _ in range(2):
        ksk, kseeds = G.relin_keygen(sk, SEED, want_resident=False)[:2]
        assert (kseeds == kseeds0).all() and (ksk == ksk0).all()
    G.close()
    # the 60-bit set of a parameter file: nothing is refused, with or without the switch
    monkeypatch.delenv("APSU_HE_SEED_REJ_CAP")
    base = Side("n1024-60")
    sk = base.G.keygen(SEED)
    idx, x = [1, 0], base.slot_values(2)
    cts0, seeds0, _ = base.query(sk, idx, x)
    assert [QS.rejection_count(sd, [int(v) for v in base.C.q[:base.L]], base.n) for sd in seeds0] == [0] * len(seeds0)
    base.close()
    monkeypatch.setenv("APSU_HE_SEED_REJ_CAP", "1")
    sd = Side("n1024-60")
    cts, seeds, _ = sd.query(sk, idx, x)
    assert (seeds == seeds0).all() and (cts == cts0).all()
    sd.close()


# ---- 5 + 6: the loop closes without the oracle as producer, and over the wire
def make_bins(sd, x, rng, max_count):
    bins = []
    for s in range(sd.n):
        c = int(rng.integers(1, max_count + 1))
        b = sorted({int(v) for v in rng.integers(1, sd.t, c)})
        c = len(b)
        if s % 3 == 0:
            b[int(rng.integers(0, c))] = int(x[s])              # the query value is a member of every third bin
        bins.append(b)
    return bins


def oracle_bundle(sd, bidx, bins, mask_vals):
    C, ps_low = sd.C, sd.p["ps_low_degree"]
    degree = max(len(b) for b in bins)
    A = np.zeros((degree + 1, sd.n), dtype=np.uint64)
    for s, b in enumerate(bins):
        A[:len(b) + 1, s] = C.polyn_with_roots(np.array(b, dtype=np.uint64))
    pci = C.plain_chain_idx(ps_low)
    coeffs = []
    for d in range(degree + 1):
        enc = C.encode(A[d])
        coeffs.append(C.plain_lift_ntt(enc, pci) if ref.coeff_is_ntt(ps_low, d) else enc)
    return dict(bundle_idx=bidx, cache_idx=0, degree=degree, A=A, coeffs=coeffs, mask_vals=mask_vals, mask=C.encode(mask_vals))


@pytest.mark.parametrize("name", ["toy", "toy-nops", "1M-1024-com"])
def test_loop_closes_on_the_engine_alone(name):
    sd = Side(name)
    C, G, n, L = sd.C, sd.G, sd.n, sd.L
    rng = np.random.default_rng(31)
    bic = sd.p["bundle_idx_count"]
    idx = list(range(bic))
    # the querier: keys and query, values on the device
    sk = G.keygen(SEED)
    ksk, kseeds, rk = G.relin_keygen(sk, SEED)
    x = sd.slot_values(bic, seed=2)
    cts, seeds, dev = sd.query(sk, idx, x, on_device=True)
    # the DB holder: BinBundles from items, masks, evaluation -- all on the device
    max_count = min(sd.p["max_items_per_bin"], 40)
    bins = {b: make_bins(sd, x[b], rng, max_count) for b in (idx if bic <= 2 else idx[:2])}
    order = sorted(bins)
    gb = [G.build_bundle(b, 0, bins[b]) for b in order]
    mbuf = torch.empty(len(order) * n, dtype=torch.int64, device="cuda")
    mask_vals, _ = G.mask_generate(77, len(order), mbuf.data_ptr())
    ptrs = [[dev.data_ptr() + ((b * sd.S + s) * 2 * L * n) * 8 for s in range(sd.S)] for b in idx]
    pw = G.compute_powers(idx, ptrs, rk, on_device=True)
    out = torch.empty((len(order), 2, n), dtype=torch.int64, device="cuda")
    G.eval_bundles(gb, pw, rk, [mbuf.data_ptr() + i * n * 8 for i in range(len(order))], out=out.data_ptr(), masks_on_device=True,
                   out_on_device=True)
    got, _, bits = G.decrypt_decode(sk[0], out.data_ptr(), count=len(order), on_device=True, want_budget=True)
    res = out.cpu().numpy().view(np.uint64).reshape(len(order), 2, 1, n)
    # the oracle as checker, fed the engine's ciphertexts and keys
    S = common.Scenario()
    S.C, S.p, S.ps_low, S.rk, S.sk = C, sd.p, sd.p["ps_low_degree"], ksk, sk
    S.targets = ref.create_powers_set(S.ps_low, sd.p["max_items_per_bin"])
    S.depth, S.nodes = ref.powers_dag(sd.p["query_powers"], S.targets)
    S.sources, S.bundle_indices = sd.sources, idx
    S.x = {b: x[b] for b in idx}
    S.src = {b: {e: np.ascontiguousarray(cts[b * sd.S + s]) for s, e in enumerate(sd.sources)} for b in idx}
    opw = common.oracle_powers(S)
    for b in idx:
        for power in S.targets:
            assert (pw.download(b, power)[0].reshape(opw[b][power].shape) == opw[b][power]).all(), (b, power)
    for i, b in enumerate(order):
        ob = oracle_bundle(sd, b, bins[b], mask_vals[i])
        assert (res[i] == common.oracle_eval(S, opw, ob)).all()
        exp = common.expected_slots(S, ob)
        assert (got[i].astype(object) == exp).all()
        member = np.array([int(x[b][s]) in bins[b][s] for s in range(n)])
        assert member[::3].all() and (got[i][member] == mask_vals[i][member]).all()
        pt, budget = C.decrypt(sk, np.ascontiguousarray(res[i]), 0)
        assert (C.decode(pt) == got[i]).all()
        assert int(bits[i]) == budget and budget > 0
    # 6: the same query as seeded SEAL objects in a framed QueryRequest: c1 and a really are their seeds' expansions
    sc = seal.SealContext(sd.js)
    parts = [(e, [sc.ct_save(sd.first, False, cts[b * sd.S + s], seed=[int(w) for w in seeds[b * sd.S + s]]) for b in idx])
             for s, e in enumerate(sd.sources)]
    msg = wire.build_query_request(0, sc.relin_keys_save(ksk, seeds=kseeds), parts)
    masks_host = mbuf.cpu().numpy().view(np.uint64).reshape(len(order), n)
    pkgs = seal.run_query_request(G, sc, msg, gb, [masks_host[i] for i in range(len(order))])
    for i in range(len(order)):
        back = sc.ct_load(wire.parse_result_package(pkgs[i])["psu_result"])
        assert back["chain_idx"] == 0 and (back["data"].reshape(2, 1, n) == res[i]).all()
    sd.close()


# ---- 7: refusals, decided on the host or reported by the call itself
def test_refusals_and_empty_calls():
    sd = Side("toy")
    G, n = sd.G, sd.n
    sk = G.keygen(SEED)
    dev = torch.zeros((sd.S, 2, sd.L, n), dtype=torch.int64, device="cuda")
    x = sd.slot_values(1)
    bad = x.copy()
    bad[0, 5] = sd.t
    with pytest.raises(ValueError):
        G.query_create(sk, [0], bad, dev.data_ptr(), seed=SEED)
    bad_dev = torch.from_numpy(bad.view(np.int64)).cuda()
    with pytest.raises(ValueError):                                       # the same value met on the device
        G.query_create(sk, [0], bad_dev.data_ptr(), dev.data_ptr(), seed=SEED, values_on_device=True)
    bad_sk = sk.copy()
    bad_sk[1, 7] = sd.C.q[1]
    with pytest.raises(ValueError):
        G.query_create(bad_sk, [0], x, dev.data_ptr(), seed=SEED)
    with pytest.raises(ValueError):
        G.relin_keygen(bad_sk, SEED)
    with pytest.raises(ValueError):
        G.query_create(sk, [sd.p["bundle_idx_count"]], x, dev.data_ptr(), seed=SEED)
    for short in (SEED[:63], list(range(7))):
        with pytest.raises(ValueError):
            G.keygen(short)
        with pytest.raises(ValueError):
            G.query_create(sk, [0], x, dev.data_ptr(), seed=short)
    assert G.query_create(sk, [], np.zeros((0, n), dtype=np.uint64), 0, seed=SEED).shape == (0, 8)     # count = 0: nothing to do
    vals, _, bits = G.decrypt_decode(sk[0], np.zeros((0, 2, 1, n), dtype=np.uint64), want_budget=True)
    assert vals.shape[0] == 0 and bits.shape[0] == 0
    assert G.keygen().shape == sk.shape and (G.keygen() != G.keygen()).any()                           # default: a fresh seed from the OS
    sd.close()
    one = Side("single-prime")                                            # no key switching: the reference creates no keys
    with pytest.raises(ValueError):
        one.G.relin_keygen(one.G.keygen(SEED), SEED)
    one.close()
