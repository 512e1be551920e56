"""CPU tier: tests/query_step_model.py -- the model test_gpu_query_steps.py holds the querier-side and decryption kernels to -- against
things it did not come from: the host codec's sample_poly_uniform, the C oracle's decrypt and add_plain, the emulation library's
samplers, and decrypt_round_coeff itself (query_side.h, the code both decryption kernels run) through emu_qs_decrypt_round on the
whole edge list the GPU test uses.  It also establishes, here and without a GPU, that the seeds, thresholds and caps of the
seed-expansion cases give the rejection counts the GPU tests rely on."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common  # noqa: E402
import emu_lib  # noqa: E402
import query_side_model as M  # noqa: E402
import query_step_model as S  # noqa: E402
from apsu_amd import seal  # noqa: E402
from oracle import pymodel, ref  # noqa: E402

u64p = C.POINTER(C.c_uint64)


def _p(a):
    return a.ctypes.data_as(u64p)


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


# ------------------------------------------------------------------------------------------------ seed expansion
def test_seed_model_at_real_thresholds_matches_the_host_codec():
    """SEAL's thresholds, the compiled cap: the model is util::sample_poly_uniform as seal_codec.cpp states it, rejections included (a
    prime just above 2^62 refuses about one word in four)"""
    n, big_q = 64, [(1 << 62) + 0x2c01, 0xffffee001]
    q = [0xffffffffc001, 0xffffee001, 0x1ffc001]
    ctx = seal.SealContext(n=n, coeff_modulus=q, plain_modulus=65537)
    big = seal.SealContext(n=n, coeff_modulus=big_q, plain_modulus=65537)
    refused = 0
    for i in range(4):
        seed = S.seed_of("codec-%d" % i)
        words, _, count, over = S.seed_expand(seed, q[:2], n)
        assert not over and (ctx.sample_poly_uniform(1, seed, 2, n) == words.astype(np.uint64)).all()
        words, rejected, count, over = S.seed_expand(seed, big_q[:1], n)
        assert not over and count == int(rejected.sum())
        assert (big.sample_poly_uniform(0, seed, 1, n) == words.astype(np.uint64)).all()
        assert (S.sample_poly_uniform(seed, big_q[:1], n) == words.astype(np.uint64)).all()
        refused += count
    assert refused > 16                                               # the replacement path really ran
    ctx.close()
    big.close()


def check_case(case, q):
    exp = case.expected(q)
    assert [e[2] for e in exp] == case.counts, case.name
    assert all(t >> 62 for t in case.thresholds), case.name            # what the step admits
    for (words, rejected, count, over), sd in zip(exp, case.seeds):
        assert over == (count > case.cap)
        raw = S.bulk_words(sd, case.limbs * case.n)
        assert len(set(raw)) == len(raw)                               # distinct: a threshold taken from them refuses exactly its rank
        for w, x in enumerate(raw):
            j, k = divmod(w, case.n)
            assert rejected[j, k] == (x >= case.thresholds[j])
            if not rejected[j, k]:
                assert words[j, k] == x % q[j]
            elif over:
                assert words[j, k] is None
            else:
                assert words[j, k] < q[j]
    return exp


def test_seed_cases_have_the_counts_the_gpu_tests_rely_on():
    q = pymodel.coeff_modulus_create(64, [40, 40, 40, 36])
    by_name = {}
    for case in S.seed_cases_small():
        by_name[case.name] = (case, check_case(case, q))
    assert by_name["no rejection"][0].counts == [0]
    case, exp = by_name["word 0 and word L n - 1"]
    assert case.counts == [2] and [tuple(x) for x in np.argwhere(exp[0][1])] == [(0, 0), (1, 63)]
    assert by_name["count == cap"][0].counts == [by_name["count == cap"][0].cap] and not by_name["count == cap"][1][0][3]
    assert by_name["count == cap + 1"][0].counts == [by_name["count == cap + 1"][0].cap + 1] and by_name["count == cap + 1"][1][0][3]
    assert by_name["cap 1, one rejection"][0].counts == [1] and not by_name["cap 1, one rejection"][1][0][3]
    case, exp = by_name["mixed overflow"]
    assert [e[3] for e in exp] == [False, True, False] and max(case.counts[0], case.counts[2]) == case.cap
    case, exp = by_name["thresholds at 2^62"]
    # three words in four are refused, and so are three in four of the replacements: the redraws alone pass one 512-word window
    assert case.counts[0] > 3 * 64 // 2 and 3 * case.counts[0] > 512 - 3 * 64
    case, exp = by_name["a threshold per limb"]
    per_limb = exp[0][1].sum(axis=1)
    assert (per_limb > 0).all() and len(set(per_limb.tolist())) == 3 and len(set(case.thresholds)) == 3
    for K, bits in ((4, [40, 40, 40, 36]), (3, [40, 40, 36]), (1, [60])):
        case = S.seed_case_key_level(64, K)
        exp = check_case(case, pymodel.coeff_modulus_create(64, bits))
        assert all(e[1].any(axis=1).all() for e in exp) or K == 1      # a rejection in every limb, the special prime's included
        assert min(case.counts) > 0


def test_rejection_rates_of_the_primes_the_fallback_tests_use():
    """the fallback tests (test_gpu_wire_query.py, test_gpu_query_side.py) need objects that refuse hundreds of words: primes just above
    2^64 / 17 do, the primes of a parameter file (2^b - c, a refused zone of 2^(64 - b) c words) practically never refuse one"""
    n = 1024
    q = S.high_rejection_primes(n, 4)
    assert all(v.bit_length() == 60 and v % (2 * n) == 1 and pymodel.is_prime(v) and 16 * v < S.W64 < 17 * v for v in q) and len(set(q)) == 4
    for v in q:
        assert 16 < S.W64 / (S.W64 - S.max_multiple(v)) < 17.1       # one word in 17
    counts = [S.rejection_count(S.seed_of("overflow-%d" % i), q, n) for i in range(8)]
    assert min(counts) > 150 and len(set(counts[:5])) >= 3
    seal_q = pymodel.coeff_modulus_create(n, [60, 60, 60, 50])
    assert all((S.W64 - S.max_multiple(v)) * n < 1 << 44 for v in seal_q)   # fewer than 2^-20 refused words expected per limb
    assert [S.rejection_count(S.seed_of("overflow-%d" % i), seal_q, n) for i in range(3)] == [0, 0, 0]


def test_seed_case_that_refills_the_cache():
    case = S.seed_case_refill()
    check_case(case, pymodel.coeff_modulus_create(1024, [60, 60, 60, 50]))
    assert case.counts[0] * 3 > 4 * 512                                # the expected redraws span several windows


def test_seed_cases_at_the_compiled_cap():
    """exactly 8192 and exactly 8193 refused words out of 16384, under thresholds the step admits (above 2^62)"""
    q = pymodel.coeff_modulus_create(8192, [56, 56, 56, 50])
    exact, over = S.seed_cases_compiled_cap()
    assert exact.cap == over.cap == S.SEED_REJ_CAP == 8192
    e = check_case(exact, q)
    assert exact.counts == [8192] and not e[0][3]
    o = check_case(over, q)
    assert over.counts == [8193] and o[0][3]


# ------------------------------------------------------------------------------------------------ decryption
def single_limb(Cx, sk, ct):
    """the oracle's own way to one limb: its rounding drops, then c0 and v = c1 s at level 0"""
    for lvl in range(Cx.first, 0, -1):
        ct = Cx.mod_switch_to_next(ct, lvl)
    v = np.ascontiguousarray(ct[1:2].copy())
    Cx.transform_to_ntt(v, 0)
    v = Cx.multiply_plain_ntt(v, np.ascontiguousarray(sk[:1]), 0)
    Cx.transform_from_ntt(v, 0)
    return ct, ct[0, 0], v[0, 0]


@pytest.mark.parametrize("kw", [dict(), dict(coeff_bits=(60,), plain_bits=9, felts=10, ps_low=0, max_items=4)])
def test_decrypt_model_matches_the_oracle_on_real_ciphertexts(kw):
    p = ref.load_params(common.toy_json(**kw))
    Cx = ref.RefContext.from_params(p)
    q0, t = Cx.q[0], Cx.t
    sk = Cx.keygen(5)
    rng = np.random.default_rng(17)
    for i in range(3):
        pt = Cx.encode(rng.integers(0, t, Cx.n, dtype=np.uint64))
        ct0, c0, v = single_limb(Cx, sk, Cx.encrypt(sk, pt, 40 + i))
        want, budget = Cx.decrypt(sk, ct0, 0)
        got, worst = S.decrypt_round_poly(c0, v, q0, t)
        assert (np.array(got, dtype=np.uint64) == want).all() and (want == pt).all()
        assert worst > 0 and S.budget_bits(worst, q0) == budget         # the C oracle runs the same loop as the engine


def test_budget_is_the_loops_definition():
    """the largest b with worst 2^b < q0 -- ceil(log2(q0 / (2 worst))) -- and the bit count of q0 for worst = 0"""
    for q0 in (3, 0xffffee001, (1 << 60) - 93, (1 << 62) - 1):
        assert S.budget_bits(0, q0) == q0.bit_length()
        worsts = {1, 2, 3, q0 >> 1, (q0 >> 1) - 1, max(1, q0 >> 2), (q0 >> 2) + 1, max(1, q0 >> 31)} | {1 << k for k in range(0, q0.bit_length() - 1, 7)}
        for w in sorted(x for x in worsts if 1 <= x <= q0 >> 1):
            b = S.budget_bits(w, q0)
            assert w << b < q0 <= w << (b + 1)
            c = 0                                                       # ceil(log2(q0 / (2 w))): the smallest c with 2^c * 2 w >= q0
            while (2 * w) << c < q0:
                c += 1
            assert b == c
            floor = (q0 // (2 * w)).bit_length() - 1                    # oracle/pymodel.py's form
            assert b - floor in (0, 1)


def decrypt_pairs():
    q1024 = pymodel.coeff_modulus_create(1024, [60, 60, 60, 50])
    toy = pymodel.coeff_modulus_create(64, [40, 40, 40, 36])
    return S.decrypt_pairs_fixed() + [(toy[0], pymodel.coeff_modulus_create(64, [17])[0]), (q1024[0], (1 << 41) - 1),
                                      (pymodel.coeff_modulus_create(64, [40, 40, 36])[2], 2)]


@pytest.mark.parametrize("q0, t", decrypt_pairs())
def test_emulated_rounding_matches_the_model_on_the_edge_list(emu, q0, t):
    xs = S.decrypt_edges(q0, t)
    assert len(xs) == 12 and all(0 <= x < q0 for x in xs)
    h = q0 >> 1
    rs = [x * t % q0 for x in xs]
    assert {0, 1 % q0, h, h + 1, q0 - 1} <= set(rs)                    # the centring's boundary is really met
    assert {0, q0 - 1} <= {(x * t + h) % q0 for x in xs}              # and the rounding's
    x = np.array(xs, dtype=np.uint64)
    out, rem = np.zeros(len(xs), dtype=np.uint64), np.zeros(len(xs), dtype=np.uint64)
    assert emu.emu_qs_decrypt_round(C.c_uint64(q0), C.c_uint64(t), _p(x), _p(out), _p(rem), len(xs)) == 0
    for i, v in enumerate(xs):
        m, r = S.decrypt_round(v, q0, t)
        assert int(out[i]) == m and int(rem[i]) == (v * t + h) % q0 and (int(rem[i]) - h) % q0 == r, (i, v)


def test_emulated_rounding_refuses_what_the_range_argument_does_not_cover(emu):
    x = np.zeros(1, dtype=np.uint64)
    o, r = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    for q0, t, v in ((1 << 62, 3, 0), ((1 << 62) - 1, 1 << 61, 0), (7, 7, 0), (7, 1, 0), (7, 2, 7)):
        x[0] = v
        assert emu.emu_qs_decrypt_round(C.c_uint64(q0), C.c_uint64(t), _p(x), _p(o), _p(r), 1) == -1


# ------------------------------------------------------------------------------------------------ the querier's side
@pytest.mark.parametrize("kw", [dict(), dict(n=1024, coeff_bits=(60, 60, 60, 50), plain_bits=17)])
def test_delta_matches_the_oracles_add_plain(kw):
    p = ref.load_params(common.toy_json(**kw))
    Cx = ref.RefContext.from_params(p)
    t, n = Cx.t, Cx.n
    pt = np.random.default_rng(3).integers(0, t, n, dtype=np.uint64)
    pt[:5] = [0, 1, (t - 1) // 2, (t + 1) // 2, t - 1]
    for lvl in range(Cx.first + 1):
        d = np.zeros((2, lvl + 1, n), dtype=np.uint64)
        Cx.add_plain(d, pt, lvl)
        q = Cx.q[:lvl + 1]
        zero = np.zeros((lvl + 1, n), dtype=np.uint64)
        want = S.enc_finish(pt, zero, np.zeros(n, dtype=np.int64), q, t)
        assert (d[0].astype(object) == want).all() and not d[1].any(), lvl


def test_slot_map_and_powers_match_the_oracles_encoder():
    Cx = ref.RefContext.from_params(ref.load_params(common.toy_json()))
    t, n = Cx.t, Cx.n
    assert S.slot_map(n) == pymodel.Model.from_bits(n, [40, 40, 40, 36], plain_bits=17).slot_map()
    vals = np.random.default_rng(5).integers(0, t, (1, n), dtype=np.uint64)
    out, flag = S.plain_powers(vals, [3], t, n)
    assert flag == 0
    # the oracle's encoder places slot i at slot_map[i] before its inverse transform: decoding the model's row gives the powers back
    M17 = pymodel.Model.from_bits(n, [40, 40, 40, 36], plain_bits=17)
    enc = np.array(M17.intt([int(v) for v in out[0]], t), dtype=np.uint64)
    assert (Cx.decode(enc).astype(object) == np.array([pow(int(v), 3, t) for v in vals[0]], dtype=object)).all()


@pytest.mark.parametrize("n", [64, 1024])
def test_sampler_models_match_the_emulation(emu, n):
    seed = bytes((13 * i + 5) & 0xFF for i in range(64))
    sd = M.seed_words(seed)
    out = np.zeros(n, dtype=np.int8)
    assert emu.emu_qs_secret(_p(sd), C.c_uint64(n), C.c_void_p(out.ctypes.data)) == 0
    assert (out.astype(np.int64) == S.secret(seed, n)).all()
    for first in (0, M.KEY_OBJECTS + 5):
        want = S.noise(seed, first, 3, n)
        for c in range(3):
            assert emu.emu_qs_noise(_p(sd), C.c_uint64(first + c), C.c_uint64(n), C.c_void_p(out.ctypes.data)) == 0
            assert (out.astype(np.int64) == want[c]).all(), (first, c)


def test_small_models_on_their_definitions():
    q = [97, 193]
    lifted = S.small_lift(np.array([[-128, -1, 0, 1, 127]]), q)
    assert lifted.tolist() == [[[66, 96, 0, 1, 30], [65, 192, 0, 1, 127]]]
    assert S.flag_monomial([[0, 0, 0], [0, 5, 0], [1, 0, 1], [1 << 63, 0, 0]]) == [0, 1, 0, 1]
    # rlk_finish: c0 + a s + e = [j == i] p s^2 in every limb
    rng = np.random.default_rng(9)
    key_q = [97, 193, 257]
    a = [[rng.integers(0, m, 4) for m in key_q] for _ in range(2)]
    e = [[rng.integers(0, m, 4) for m in key_q] for _ in range(2)]
    s = [rng.integers(0, m, 4) for m in key_q]
    c0 = S.rlk_finish(a, s, e, key_q)
    for i in range(2):
        for j, m in enumerate(key_q):
            for k in range(4):
                lhs = (int(c0[i, j, k]) + int(a[i][j][k]) * int(s[j][k]) + int(e[i][j][k])) % m
                assert lhs == ((257 * int(s[j][k]) ** 2) % m if j == i else 0)
