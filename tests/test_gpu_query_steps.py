"""GPU tier: every launcher of the querier's side and of the decryption, one launch at a time, bit for bit against the integer model.

apsu_he_debug_run_step (the steps from seed_expand on, apsu_amd/csrc/engine_query_steps.cpp) puts chosen words in front of ONE call of
the launcher engine_query.cpp calls, with the context's own level and key blocks and its slot map; tests/query_step_model.py states
the same step on Python integers (held to the host codec, the C oracle and the emulation by test_query_step_model_cpu.py, which also
establishes the rejection counts of the seed cases used here).  The end-to-end tests of this family are exact but cannot choose the
words a kernel sees; these do: rejection lists empty, at their cap and one past it, replacement draws that are themselves refused
across refills of the stream cache, the rounding of the decryption at the ends of its range and on both sides of every boundary, the
noise maximum at a chosen lane, wave and workgroup, every signed byte, every crossing of 0, 1 and q - 1.  No tolerance anywhere.
"""
import numpy as np
import pytest

import apsu_amd
import common
import query_side_model as M
import query_step_model as S
from apsu_amd.engine import STEP_ACCUMULATE, STEP_KEY
from oracle import ref

pytestmark = pytest.mark.gpu

W64 = 1 << 64
POISON = 0xA5A5A5A5A5A5A5A5                     # above every modulus: never a word a kernel may write
SEED = bytes((13 * i + 5) & 0xFF for i in range(64))

PARAMS = {
    "toy": dict(),
    "toy-k3": dict(coeff_bits=(40, 40, 36)),
    "toy-k2": dict(coeff_bits=(40, 36)),
    "n1024": dict(n=1024, coeff_bits=(60, 60, 60, 50), plain_bits=17),
    "single-prime": dict(n=64, coeff_bits=(60,), plain_bits=9, felts=10, ps_low=0, max_items=4),
    "n8192": dict(n=8192, coeff_bits=(56, 56, 56, 50), plain_bits=22),
}
_CTX = {}


@pytest.fixture(scope="module")
def ctx():
    def get(name):
        if name not in _CTX:
            _CTX[name] = apsu_amd.HeContext(common.toy_json(**PARAMS[name]))
        return _CTX[name]
    yield get
    for G in _CTX.values():
        G.close()
    _CTX.clear()


def u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=object).astype(np.uint64))


def s64(a):
    """signed values as sign-extended 64-bit words"""
    return np.ascontiguousarray(np.asarray(a, dtype=np.int64)).view(np.uint64)


def poison(*shape):
    return np.full(shape, POISON, dtype=np.uint64)


def same(got, want, what):
    got = np.asarray(got)
    want = u64(want).reshape(got.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), "%s: %d words differ, first at %s: got %#x, want %#x" % (what, len(bad), tuple(bad[0]), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


# ================================================================ seed_expand
def run_seed_case(G, case, cap=None):
    L, n, batch = case.limbs, case.n, len(case.seeds)
    assert n == G.n and L <= G.K
    chain = -1 if L == G.K else L - 1
    out, ctr = poison(batch, L, n), poison(batch + 1)
    G.debug_run_step("seed_expand", chain, ins=[u64(case.seeds).reshape(-1), u64(case.thresholds)], outs=[out, ctr], terms=case.cap if cap is None else cap,
                     batch=batch)
    return out, ctr


def check_seed_case(G, case):
    out, ctr = run_seed_case(G, case)
    exp = case.expected(G.q)
    assert [e[2] for e in exp] == case.counts                      # (the CPU tier has established them)
    for b, (words, rejected, count, over) in enumerate(exp):
        # (an overflowed object's refused positions stay unwritten)
        want = [[POISON if w is None else w for w in row] for row in words]
        assert over == any(w is None for row in words for w in row)
        same(out[b], want, "%s: object %d" % (case.name, b))
        assert int(ctr[b]) == (count if over else 0), (case.name, b, int(ctr[b]))
    assert int(ctr[-1]) == (1 if any(e[3] for e in exp) else 0), case.name
    return exp


@pytest.mark.parametrize("case", S.seed_cases_small(), ids=lambda c: c.name)
def test_seed_expand_known_counts(ctx, case):
    G = ctx("toy")
    exp = check_seed_case(G, case)
    if any(e[3] for e in exp):
        # the call after an overflowing one, with lists of its own and room for everything: every object complete and exact
        out, ctr = run_seed_case(G, case, cap=S.SEED_REJ_CAP)
        for b, sd in enumerate(case.seeds):
            words = S.seed_expand(sd, G.q[:case.limbs], case.n, case.thresholds)[0]
            same(out[b], words, "%s again: object %d" % (case.name, b))
        assert not ctr.any()


@pytest.mark.parametrize("name", ["toy", "toy-k3", "single-prime"])
def test_seed_expand_key_level(ctx, name):
    """all K limbs: the moduli-only view where the key level is no data level (K - 1 > first_chain_idx), the level block itself otherwise"""
    G = ctx(name)
    check_seed_case(G, S.seed_case_key_level(G.n, G.K))
    # and under SEAL's own thresholds, as the engine runs it
    sd = S.seed_of("real-%s" % name)
    case = S.SeedCase("real thresholds", G.n, G.K, [sd], [S.max_multiple(q) for q in G.q], S.SEED_REJ_CAP, [S.seed_expand(sd, G.q, G.n)[2]])
    check_seed_case(G, case)


def test_seed_expand_redraws_across_cache_refills(ctx):
    check_seed_case(ctx("n1024"), S.seed_case_refill())


def test_seed_expand_at_the_compiled_cap(ctx):
    G = ctx("n8192")
    exact, over = S.seed_cases_compiled_cap()
    e = check_seed_case(G, exact)
    assert e[0][2] == 8192 and not e[0][3]
    o = check_seed_case(G, over)
    assert o[0][2] == 8193 and o[0][3]


# ================================================================ decrypt_round
def run_decrypt(G, ct, v, q0, t):
    """both launchers on the same words -> (values, worst); the two value arrays must be identical"""
    batch, n = v.shape
    plain, with_budget, worst = poison(batch, n), poison(batch, n), poison(batch)
    ins = [ct, v, u64([q0, t])]
    G.debug_run_step("decrypt_round", 0, ins=ins, outs=[plain], batch=batch)
    G.debug_run_step("decrypt_round", 0, ins=ins, outs=[with_budget, worst], flags=STEP_ACCUMULATE, batch=batch)
    assert (plain == with_budget).all()
    return plain, worst


def decrypt_pairs(ctx, name):
    G = ctx(name)
    pairs = [(G.q[0], G.t)]
    if name in ("toy", "n1024"):
        pairs += S.decrypt_pairs_fixed()
    if name == "n1024":
        pairs.append((G.q[1], (1 << 41) - 1))
    if name == "toy-k3":
        assert G.q[2].bit_length() == 36
        pairs.append((G.q[2], 2))
    return G, pairs


@pytest.mark.parametrize("name", ["toy", "toy-k3", "n1024", "single-prime"])
def test_decrypt_round_edges(ctx, name):
    G, pairs = decrypt_pairs(ctx, name)
    n = G.n
    rng = np.random.default_rng(41)
    for q0, t in pairs:
        xs = S.decrypt_edges(q0, t)
        c0, v = [0] * n, [0] * n
        for i, x in enumerate(xs):                                  # each x split both ways round
            c0[2 * i], v[2 * i] = x, 0
            c0[2 * i + 1], v[2 * i + 1] = q0 - 1, (x + 1) % q0
        for k in range(2 * len(xs), n):                             # the rest: any residues
            c0[k], v[k] = int(rng.integers(0, min(q0, 1 << 62))), int(rng.integers(0, min(q0, 1 << 62)))
        ct = np.stack([u64(c0), rng.integers(0, 1 << 63, n, dtype=np.uint64)])[None]
        got, worst = run_decrypt(G, np.ascontiguousarray(ct), u64(v)[None], q0, t)
        want, w = S.decrypt_round_poly(c0, v, q0, t)
        for i, x in enumerate(xs):
            assert want[2 * i] == want[2 * i + 1] == S.decrypt_round(x, q0, t)[0]
        same(got[0], want, "decrypt_round (%#x, %#x)" % (q0, t))
        assert int(worst[0]) == w, (hex(q0), hex(t), int(worst[0]), w)


@pytest.mark.parametrize("name, places", [("n1024", (0, 63, 64, 255, 256, 1023)), ("toy", (0, 63))])
def test_decrypt_round_worst_by_place(ctx, name, places):
    """the one coefficient with a distance sits at a chosen lane, wave and workgroup; every other one gives 0.  At n = 64 three of the
    workgroup's four waves hold no coefficient."""
    G = ctx(name)
    n, q0, t = G.n, G.q[0], G.t
    inv, h = pow(t, -1, q0), q0 >> 1
    c0 = np.zeros((len(places), 2, n), dtype=np.uint64)
    v = np.zeros((len(places), n), dtype=np.uint64)
    want = []
    for b, p in enumerate(places):                                  # one ciphertext per place, a different maximum each
        r = h - 3 * b if b % 2 == 0 else h + 1 + 3 * b              # either side of the centring
        c0[b, 0, p] = r * inv % q0
        want.append(S.distance(r, q0))
    got, worst = run_decrypt(G, c0, v, q0, t)
    assert [int(w) for w in worst] == want
    for b in range(len(places)):
        same(got[b], S.decrypt_round_poly(c0[b, 0], v[b], q0, t)[0], "place %d" % places[b])


def test_decrypt_round_worst_three_ciphertexts_one_noiseless(ctx):
    G = ctx("n1024")
    n, q0, t = G.n, G.q[0], G.t
    inv = pow(t, -1, q0)
    rng = np.random.default_rng(43)
    c0 = np.zeros((3, 2, n), dtype=np.uint64)
    v = np.zeros((3, n), dtype=np.uint64)
    # 0: distances everywhere, the largest in the last workgroup; 1: all zeros; 2: small distances and one large in wave 1 of workgroup 2
    r0 = [int(x) for x in rng.integers(0, q0 >> 3, n)]
    r0[1000] = (q0 >> 1) + 1
    r2 = [int(x) for x in rng.integers(0, 1 << 20, n)]
    r2[2 * 256 + 64 + 5] = q0 - (1 << 30)
    for b, rs in ((0, r0), (2, r2)):
        x = [r * inv % q0 for r in rs]
        split = [int(s) for s in rng.integers(0, q0, n)]            # x = c0 + v with both halves busy
        c0[b, 0] = u64(split)
        v[b] = u64([(xx - s) % q0 for xx, s in zip(x, split)])
    got, worst = run_decrypt(G, c0, v, q0, t)
    assert [int(w) for w in worst] == [q0 - ((q0 >> 1) + 1), 0, 1 << 30]
    for b in range(3):
        m, w = S.decrypt_round_poly(c0[b, 0], v[b], q0, t)
        same(got[b], m, "ciphertext %d" % b)
        assert int(worst[b]) == w


def test_budget_of_decrypt_decode_is_the_loops_definition(ctx):
    """apsu_he_decrypt_decode's budget = the largest b with worst 2^b < q_0 (the bit count of q_0 for worst = 0), worst taken from the
    step on the same ciphertexts"""
    G = ctx("toy")
    Cx = ref.RefContext.from_params(ref.load_params(common.toy_json()))
    n, q0, t = G.n, G.q[0], G.t
    sk = G.keygen(SEED)
    rng = np.random.default_rng(47)
    cts = []
    for i in range(3):                                              # real ciphertexts, brought to one limb by the oracle's rounding drops
        ct = Cx.encrypt(sk, Cx.encode(rng.integers(0, t, n, dtype=np.uint64)), 70 + i)
        for lvl in range(Cx.first, 0, -1):
            ct = Cx.mod_switch_to_next(ct, lvl)
        cts.append(ct)
    noiseless = np.zeros((2, 1, n), dtype=np.uint64)                # c1 = 0: x = c0
    noisy = noiseless.copy()
    noisy[0, 0, 17] = (q0 >> 1) * pow(t, -1, q0) % q0
    cts = np.ascontiguousarray(np.stack(cts + [noiseless, noisy]))
    v = np.ascontiguousarray(cts[:, 1].copy())                      # v = c1 s in coefficient form, [count][1][n]
    Cx.transform_to_ntt(v, 0)
    v = Cx.multiply_plain_ntt(v, np.ascontiguousarray(sk[:1]), 0)
    Cx.transform_from_ntt(v, 0)
    _, worst = run_decrypt(G, np.ascontiguousarray(cts.reshape(-1, 2, n)), np.ascontiguousarray(v.reshape(-1, n)), q0, t)
    bits = G.decrypt_decode(sk[0], cts, want_budget=True)[2]
    assert [int(b) for b in bits] == [S.budget_bits(int(w), q0) for w in worst]
    assert int(worst[3]) == 0 and int(bits[3]) == q0.bit_length() and int(worst[4]) == q0 >> 1 and int(bits[4]) == 1
    assert all(0 < int(w) < q0 >> 4 for w in worst[:3])


# ================================================================ plain_powers
EXPONENTS7 = [0, 1, 2, 3, 1 << 16, (1 << 16) - 1, (1 << 32) - 1]


def run_powers(G, vals, exps):
    batch, n, Sn = len(vals), G.n, len(exps)
    out, flag = poison(batch * Sn, n), poison(1)
    G.debug_run_step("plain_powers", 0, ins=[u64(vals), u64(exps)], outs=[out, flag], batch=batch)
    want, wflag = S.plain_powers(vals, exps, G.t, n)
    same(out, want, "plain_powers %s" % (exps,))
    assert int(flag[0]) == wflag
    return wflag


@pytest.mark.parametrize("name", ["toy", "n1024"])
def test_plain_powers(ctx, name):
    G = ctx(name)
    n, t = G.n, G.t
    rng = np.random.default_rng(53)
    vals = [[int(x) for x in rng.integers(0, t, n)] for _ in range(2)]
    vals[0][:4] = [0, 1, 2, t - 1]
    vals[1][-4:] = [t - 1, 2, 1, 0]
    assert run_powers(G, vals, EXPONENTS7) == 0                     # batch = 2, nothing bad: the flag stays clean
    for exps in ([0], [1 << 31], [(1 << 31) - 1]):                  # S = 1
        assert run_powers(G, vals[:1], exps) == 0
    for first, last in ((t, W64 - 1), (W64 - 1, t)):                # a bad value at the first and at the last slot
        bad = [row[:] for row in vals]
        bad[0][0], bad[1][n - 1] = first, last
        assert run_powers(G, bad, EXPONENTS7) == 1
        assert run_powers(G, bad[1:], [0, 5]) == 1


# ================================================================ the samplers
@pytest.mark.parametrize("name", ["toy", "n1024"])
def test_sample_small(ctx, name):
    G = ctx(name)
    n = G.n
    sd = M.seed_words(SEED)
    out = poison(n)
    G.debug_run_step("sample_small", 0, ins=[sd], outs=[out])
    assert (out.view(np.int64) == S.secret(SEED, n)).all()
    for first in (0, M.KEY_OBJECTS + 5):
        out = poison(3, n)
        G.debug_run_step("sample_small", 0, ins=[sd], outs=[out], flags=STEP_KEY, e0=first, batch=3)
        assert (out.view(np.int64) == S.noise(SEED, first, 3, n)).all(), first


# ================================================================ small_lift
@pytest.mark.parametrize("name", ["toy", "n1024", "single-prime"])
def test_small_lift_every_signed_byte(ctx, name):
    G = ctx(name)
    n, K = G.n, G.K
    every = np.arange(-128, 128, dtype=np.int64)
    for start in range(0, 256, 2 * n):                              # two rows per launch until every value has been seen
        small = np.stack([np.resize(np.roll(every, -start), n), np.resize(np.roll(every, -(start + n)), n)])
        for limbs in sorted({1, K}):
            out = poison(2, limbs, n)
            G.debug_run_step("small_lift", 0, ins=[s64(small)], outs=[out], polys=limbs, batch=2)
            same(out, S.small_lift(small, G.q[:limbs]), "small_lift %d limbs" % limbs)


# ================================================================ enc_finish
@pytest.mark.parametrize("name", ["toy", "toy-k3", "n1024", "single-prime"])
def test_enc_finish(ctx, name):
    G = ctx(name)
    n, t = G.n, G.t
    rng = np.random.default_rng(59)
    ms = [0, 1, (t - 1) // 2, (t + 1) // 2, t - 1]
    es = [-128, -21, -1, 0, 1, 21, 127]
    combos = [(m, e, vi) for m in ms for e in es for vi in range(3)]
    batch = 3
    assert len(combos) <= batch * n
    for c in range(G.first_chain_idx + 1):
        q = G.q[:c + 1]
        L = len(q)
        pt = [int(x) for x in rng.integers(0, t, batch * n)]
        e = [int(x) for x in rng.integers(-128, 128, batch * n)]
        v = [[int(x) for x in rng.integers(0, qj, batch * n)] for qj in q]
        for i, (m, ek, vi) in enumerate(combos):
            pt[i], e[i] = m, ek
            for j, qj in enumerate(q):
                v[j][i] = (0, 1, qj - 1)[vi]
        pt, e = np.array(pt, dtype=object).reshape(batch, n), np.array(e).reshape(batch, n)
        v = np.array(v, dtype=object).reshape(L, batch, n).transpose(1, 0, 2)
        cts = poison(batch, 2, L, n)
        G.debug_run_step("enc_finish", c, ins=[u64(pt), u64(v), s64(e)], outs=[cts], batch=batch)
        assert (cts[:, 1] == POISON).all(), "a c1 half was written"
        for b in range(batch):
            same(cts[b, 0], S.enc_finish(pt[b], v[b], e[b], q, t), "enc_finish level %d ciphertext %d" % (c, b))


# ================================================================ rlk_finish
@pytest.mark.parametrize("name", ["toy-k2", "toy"])
def test_rlk_finish(ctx, name):
    G = ctx(name)
    n, K = G.n, G.K
    assert K == (2 if name == "toy-k2" else 4)
    rng = np.random.default_rng(61)
    a = np.empty((K - 1, K, n), dtype=object)
    e = np.empty((K - 1, K, n), dtype=object)
    s = np.empty((K, n), dtype=object)
    for j, q in enumerate(G.q):
        s[j] = [int(x) for x in rng.integers(0, q, n)]
        for i in range(K - 1):
            a[i, j] = [int(x) for x in rng.integers(0, q, n)]
            e[i, j] = [int(x) for x in rng.integers(0, q, n)]
        k = 0
        for av in (0, 1, q - 1):                                    # crossed, on every (i, j): s is shared by the keys, so the cross is per limb
            for sv in (0, 1, q - 1):
                for evv in (0, 1, q - 1):
                    s[j, k] = sv
                    a[:, j, k], e[:, j, k] = av, evv
                    k += 1
    ksk = poison(K - 1, 2, K, n)
    ksk[:, 1] = u64(a)
    G.debug_run_step("rlk_finish", 0, ins=[u64(s), u64(e)], outs=[ksk])
    same(ksk[:, 1], a, "the a halves")
    same(ksk[:, 0], S.rlk_finish(a, s, e, G.q), "rlk_finish")


# ================================================================ flag_monomial
def test_flag_monomial(ctx):
    G = ctx("n1024")
    n = G.n
    places = [(), (0,), (255,), (256,), (n - 1,), (0, 1), (0, 256), (255, n - 1)]
    pt = np.zeros((len(places), n), dtype=np.uint64)
    for b, ps in enumerate(places):
        for i, p in enumerate(ps):
            pt[b, p] = (1, 1 << 63)[i]
    out = poison(len(places))
    G.debug_run_step("flag_monomial", 0, ins=[pt], outs=[out], batch=len(places))
    assert [int(x) for x in out] == S.flag_monomial(pt) == [0, 1, 1, 1, 1, 0, 0, 0]
    G = ctx("toy")                                                  # n = 64: one stride of the loop, three quarters of the lanes idle
    places = [(), (0,), (63,), (0, 1), (0, 63)]
    pt = np.zeros((5, 64), dtype=np.uint64)
    for b, ps in enumerate(places):
        for p in ps:
            pt[b, p] = G.t - 1
    out = poison(5)
    G.debug_run_step("flag_monomial", 0, ins=[pt], outs=[out], batch=5)
    assert [int(x) for x in out] == S.flag_monomial(pt) == [0, 1, 1, 0, 0]


# ================================================================ refusals
def test_refusals(ctx, monkeypatch):
    G = ctx("toy")
    n, K, t, q = G.n, G.K, G.t, G.q
    sd = u64(S.seed_of("refused"))
    ok_th = u64([1 << 62] * 3)

    def refused(step, chain, ins, outs, **kw):
        before = [o.copy() for o in outs]
        with pytest.raises(ValueError):
            G.debug_run_step(step, chain, ins=ins, outs=outs, **kw)
        for o, b in zip(outs, before):
            assert (o == b).all()                                   # nothing was launched, nothing copied back

    seed_outs = lambda batch=1, L=3: [poison(batch, L, n), poison(batch + 1)]
    refused("seed_expand", 2, [sd, u64([1 << 62, (1 << 62) - 1, 1 << 62])], seed_outs(), terms=16)      # a threshold below 2^62: the redraw loop might not end
    refused("seed_expand", 2, [sd, u64([0] * 3)], seed_outs(), terms=16)
    refused("seed_expand", 2, [sd, ok_th], seed_outs(), terms=0)
    refused("seed_expand", 2, [sd, ok_th], seed_outs(), terms=8193)
    refused("seed_expand", 7, [sd, ok_th], seed_outs(), terms=16)                                      # no level
    refused("seed_expand", 2, [sd, ok_th[:2]], seed_outs(), terms=16)
    refused("seed_expand", 2, [sd[:7], ok_th], seed_outs(), terms=16)
    refused("seed_expand", 2, [sd, ok_th], [poison(1, 3, n), poison(1)], terms=16)
    refused("seed_expand", 2, [sd, ok_th], seed_outs(), terms=16, batch=0)
    refused("seed_expand", 2, [np.tile(sd, 65), ok_th], seed_outs(65), terms=16, batch=65)

    ct, v = np.zeros((1, 2, n), dtype=np.uint64), np.zeros((1, n), dtype=np.uint64)
    for flags, outs in ((0, lambda: [poison(1, n)]), (STEP_ACCUMULATE, lambda: [poison(1, n), poison(1)])):
        for q0, tt in ((q[0], q[0]), (q[0], q[0] + 1), (1 << 62, 5), ((1 << 62) - 1, 1 << 61), (q[0], 1), (q[0], 0)):
            refused("decrypt_round", 0, [ct, v, u64([q0, tt])], outs(), flags=flags)
        bad = ct.copy()
        bad[0, 0, n - 1] = q[0]
        refused("decrypt_round", 0, [bad, v, u64([q[0], t])], outs(), flags=flags)
        bad = v.copy()
        bad[0, 0] = q[0]
        refused("decrypt_round", 0, [ct, bad, u64([q[0], t])], outs(), flags=flags)
        refused("decrypt_round", 0, [ct, v, u64([q[0]])], outs(), flags=flags)
    refused("decrypt_round", 0, [ct, v, u64([q[0], t])], [poison(1, n), poison(2)], flags=STEP_ACCUMULATE)

    vals = np.zeros((1, n), dtype=np.uint64)
    refused("plain_powers", 0, [vals, u64([1, 1 << 32])], [poison(2, n), poison(1)])
    refused("plain_powers", 0, [vals, u64([1, 2])], [poison(1, n), poison(1)])
    refused("plain_powers", 0, [vals, u64([])], [poison(1, n), poison(1)])

    refused("sample_small", 0, [sd], [poison(2, n)], batch=2)                                          # the secret is one polynomial
    refused("sample_small", 0, [sd], [poison(1, n)], e0=1)
    refused("sample_small", 0, [sd], [poison(2, n)], flags=STEP_KEY, e0=M.MAX_OBJECTS - 1, batch=2)
    refused("sample_small", 0, [sd[:7]], [poison(1, n)])

    small = np.zeros((1, n), dtype=np.int64)
    for badv in (128, -129, 255):
        x = small.copy()
        x[0, 3] = badv
        refused("small_lift", 0, [s64(x)], [poison(1, 1, n)], polys=1)
    refused("small_lift", 0, [s64(small)], [poison(1, 1, n)], polys=0)
    refused("small_lift", 0, [s64(small)], [poison(1, K + 1, n)], polys=K + 1)

    pt, vv, e = np.zeros((1, n), dtype=np.uint64), np.zeros((1, 2, n), dtype=np.uint64), np.zeros((1, n), dtype=np.int64)
    x = pt.copy()
    x[0, 0] = t
    refused("enc_finish", 1, [x, vv, s64(e)], [poison(1, 2, 2, n)])
    x = vv.copy()
    x[0, 1, 5] = q[1]
    refused("enc_finish", 1, [pt, x, s64(e)], [poison(1, 2, 2, n)])
    x = e.copy()
    x[0, 9] = 200
    refused("enc_finish", 1, [pt, vv, s64(x)], [poison(1, 2, 2, n)])
    refused("enc_finish", 3, [pt, vv, s64(e)], [poison(1, 2, 2, n)])                                   # the key level is no data level
    refused("enc_finish", 1, [pt, vv, s64(e)], [poison(1, 2, 3, n)])

    s, ee, ksk = np.zeros((K, n), dtype=np.uint64), np.zeros((K - 1, K, n), dtype=np.uint64), np.zeros((K - 1, 2, K, n), dtype=np.uint64)
    x = s.copy()
    x[2, 0] = q[2]
    refused("rlk_finish", 0, [x, ee], [ksk.copy()])
    x = ee.copy()
    x[1, 3, 0] = q[3]
    refused("rlk_finish", 0, [s, x], [ksk.copy()])
    x = ksk.copy()
    x[0, 1, 1, 7] = q[1]                                            # an a half is read: canonical
    refused("rlk_finish", 0, [s, ee], [x])
    x = ksk.copy()
    x[0, 0, 1, 7] = POISON                                          # a c0 half is only written: any word
    G.debug_run_step("rlk_finish", 0, ins=[s, ee], outs=[x])
    assert not x.any()
    one = ctx("single-prime")
    with pytest.raises(ValueError):
        one.debug_run_step("rlk_finish", 0, ins=[np.zeros((1, 64), dtype=np.uint64), np.zeros(0, dtype=np.uint64)], outs=[np.zeros(0, dtype=np.uint64)])

    refused("flag_monomial", 0, [np.zeros((2, n), dtype=np.uint64)], [poison(1)])
    refused("flag_monomial", 0, [np.zeros((1, n), dtype=np.uint64)], [poison(2)])

    # the switch behind the engine's own cap: outside 1 .. 8192 no context is created
    for bad in ("0", "8193", "-1", ""):
        monkeypatch.setenv("APSU_HE_SEED_REJ_CAP", bad)
        with pytest.raises(ValueError):
            apsu_amd.HeContext(common.toy_json())
    monkeypatch.delenv("APSU_HE_SEED_REJ_CAP")
