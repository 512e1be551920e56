"""CPU tier: the big-integer step model (tests/kernel_step_model.py) composed with the oracle's transforms equals the C oracle.

multiply / square = ext -> NTT -> tensor -> INTT -> finish; relinearize = inner product -> INTT -> mod-down; mod_switch_to_next; the
sums of individually rounded terms that eval_patstock takes; the evaluation's tail.  Every RAW variant equals the plain one once the
twist is applied.  Chains: one whose levels all take the unrolled kernels (L = nB <= 3), one with L = 4, one generic (L = 5), and one
with nB = L + 1 (41-bit plain modulus), at n = 64 and n = 256.  This is what makes a mismatch of the GPU step tests mean the kernel.
The transforms are oracle/pymodel.py's definition (evaluation at psi^(2 brv(i) + 1)), held to the C oracle's below."""
import numpy as np
import pytest

import kernel_step_model as ksm
from kernel_step_model import O, U
from oracle import pymodel, ref

CHAINS = {
    "unrolled": dict(bits=[60, 60, 60, 60], plain_bits=17, shapes=[(3, 3), (2, 2), (1, 1)]),
    "L4": dict(bits=[50, 50, 50, 50, 50], plain_bits=17, shapes=[(4, 4), (3, 3), (2, 2), (1, 1)]),
    "generic": dict(bits=[50] * 6, plain_bits=17, shapes=[(5, 5), (4, 4), (3, 3), (2, 2), (1, 1)]),
    "nB=L+1": dict(bits=[60, 60, 60], plain_bits=41, shapes=[(2, 3), (1, 2)]),
}
_CTX = {}


def context(n, chain):
    """(C oracle, step model) of one chain, built once"""
    if (n, chain) not in _CTX:
        spec = CHAINS[chain]
        C = ref.RefContext(n, spec["bits"], 0, spec["plain_bits"])
        M = pymodel.Model(n, [int(v) for v in C.q], int(C.t))
        S = ksm.StepModel.from_pymodel(M)
        assert [(lv.L, lv.nB) for lv in reversed(S.lv)] == spec["shapes"], chain
        _CTX[(n, chain)] = (C, S)
    return _CTX[(n, chain)]


_POINTS = {}


def points(S, m, inverse=False):
    """psi^(2 brv(i) + 1), or their inverses"""
    if (S.n, m, inverse) not in _POINTS:
        n, logn = S.n, S.n.bit_length() - 1
        psi = pymodel.minimal_primitive_root(2 * n, m)
        if inverse:
            psi = pow(psi, -1, m)
        _POINTS[(S.n, m, inverse)] = np.array([pow(psi, 2 * pymodel.brv(i, logn) + 1, m) for i in range(n)], dtype=object)
    return _POINTS[(S.n, m, inverse)]


def ntt(S, a, m):
    x, acc = points(S, m), 0
    for c in a[::-1]:
        acc = (acc * x + c) % m
    return acc


def intt(S, A, m, raw=False):
    """inverse of ntt(); raw: without n^-1 psi^-k, as a RAW inverse transform leaves it (plus a multiple of m, to be no residue)"""
    xinv, cur, out = points(S, m, inverse=True), A, []
    for _ in range(S.n):
        out.append(sum(cur) % m)
        cur = cur * xinv % m
    out = np.array(out, dtype=object)
    # sum_i A_i x_i^-j = n c_j; x_i^-j = psi^-j (psi^2)^(-brv(i) j): the cyclic part is what a RAW transform returns
    if raw:
        psi = pymodel.minimal_primitive_root(2 * S.n, m)
        tw = np.array([pow(psi, j, m) for j in range(S.n)], dtype=object)
        return out * tw % m + m * (np.arange(S.n) % 3).astype(object)
    return out * pow(S.n, -1, m) % m


def rand_ct(rng, q, n, polys=2):
    return np.stack([np.stack([rng.integers(0, m, n, dtype=np.uint64) for m in q]) for _ in range(polys)])


def model_product(S, c, a, b, raw):
    """(d [3][E][n] in coefficient form -- raw words where asked --, the finished product [3][L][n])"""
    lv = S.lv[c]
    ea = [[ntt(S, x, m) for x, m in zip(S.behz_ext(c, list(O(p))), lv.ext)] for p in a]
    eb = [[ntt(S, x, m) for x, m in zip(S.behz_ext(c, list(O(p))), lv.ext)] for p in b]
    d = [[intt(S, x, m, raw) for x, m in zip(p, lv.ext)] for p in S.tensor(c, ea, eb)]
    return d, [S.behz_finish(c, [p], raw) for p in d]


PARAMS = [(n, chain) for n in (64, 256) for chain in CHAINS]


@pytest.mark.parametrize("n,chain", PARAMS)
def test_transforms_of_the_model_are_the_oracles(n, chain):
    C, S = context(n, chain)
    rng = np.random.default_rng(n)
    x = rand_ct(rng, C.q[:C.first + 1], n, 1)
    want = x.copy()
    C.transform_to_ntt(want, C.first)
    got = U([[ntt(S, O(l), int(m)) for l, m in zip(x[0], C.q)]])
    assert (got == want).all()
    back = U([[intt(S, O(l), int(m)) for l, m in zip(want[0], C.q)]])
    assert (back == x).all()
    for l, m in zip(want[0], C.q):                                    # a raw word stands for the residue the twist gives
        assert (S.twist(intt(S, O(l), int(m), raw=True), int(m)) == intt(S, O(l), int(m))).all()


@pytest.mark.parametrize("n,chain", PARAMS)
def test_multiply_and_square_are_ext_tensor_finish(n, chain):
    C, S = context(n, chain)
    rng = np.random.default_rng(1000 + n)
    c = C.first if n == 64 else max(C.first - 1, 0)                    # the first level at n = 64, one below it at n = 256
    q = C.q[:c + 1]
    a, b = rand_ct(rng, q, n), rand_ct(rng, q, n)
    for x, y, want in ((a, b, C.multiply(a, b, c)), (a, a, C.square(a, c))):
        _, got = model_product(S, c, x, y, raw=False)
        assert (U(got) == want).all()
        _, got_raw = model_product(S, c, x, y, raw=True)
        assert (U(got_raw) == want).all()


@pytest.mark.parametrize("n,chain", PARAMS)
def test_summed_product_is_the_sum_of_the_finished_products(n, chain):
    """tensor_sum + finish_sum on three products == the oracle's multiply per product, added (bin_bundle.cpp:273,303)"""
    C, S = context(n, chain)
    rng = np.random.default_rng(2000 + n)
    c = min(C.first, 1)
    lv, q = S.lv[c], C.q[:c + 1]
    terms = 3
    pairs = [(rand_ct(rng, q, n), rand_ct(rng, q, n)) for _ in range(terms)]
    want = np.zeros((3, c + 1, n), dtype=object)
    for x, y in pairs:
        want = want + O(C.multiply(x, y, c))
    want = U([[l % int(m) for l, m in zip(p, q)] for p in want])
    ea = [[[ntt(S, v, m) for v, m in zip(S.behz_ext(c, list(O(p))), lv.ext)] for p in x] for x, _ in pairs]
    eb = [[[ntt(S, v, m) for v, m in zip(S.behz_ext(c, list(O(p))), lv.ext)] for p in y] for _, y in pairs]
    dq, bs = S.tensor_sum(c, ea, eb)
    for raw in (False, True):
        dqc = [[[intt(S, v, m, raw) for v, m in zip(p, lv.q)] for p in term] for term in dq]
        bsc = [[intt(S, v, m, raw) for v, m in zip(p, lv.Bsk)] for p in bs]
        got = [S.behz_finish_sum(c, [term[p] for term in dqc], bsc[p], raw) for p in range(3)]
        assert (U(got) == want).all(), raw
    # ... and the per-term finish of the same products, accumulated (launch_behz_finish with terms > 1)
    per = [S.tensor(c, x, y) for x, y in zip(ea, eb)]
    dc = [[[intt(S, v, m) for v, m in zip(p, lv.ext)] for p in term] for term in per]
    got = [S.behz_finish(c, [term[p] for term in dc]) for p in range(3)]
    assert (U(got) == want).all()


@pytest.mark.parametrize("n,chain", PARAMS)
def test_relinearize_is_inner_product_and_rounded_division(n, chain):
    C, S = context(n, chain)
    rng = np.random.default_rng(3000 + n)
    c = C.first if n == 64 else max(C.first - 1, 0)
    L, q = c + 1, C.q[:c + 1]
    rk = C.gen_relin_keys(C.keygen(7), 8)
    ct3 = rand_ct(rng, q, n, 3)
    want = C.relinearize(ct3, rk, c)
    mods = S.acc_mods(c)
    tdec = [[ntt(S, O(ct3[2][J]) % m, m) for J in range(L)] for m in mods]
    acc = S.ks_inner(c, tdec, O(rk))
    for raw in (False, True):
        accc = [[intt(S, v, m, raw) for v, m in zip(comp, mods)] for comp in acc]
        got = S.ks_moddown(c, accc, [list(O(p)) for p in ct3[:2]], raw)
        assert (U(got) == want).all(), raw


@pytest.mark.parametrize("n,chain", PARAMS)
def test_mod_switch_and_the_fused_drop(n, chain):
    C, S = context(n, chain)
    rng = np.random.default_rng(4000 + n)
    for c in range(C.first, 0, -1):
        ct = rand_ct(rng, C.q[:c + 1], n)
        want = C.mod_switch_to_next(ct, c)
        assert (U([S.modswitch(c, list(O(p))) for p in ct]) == want).all()
        rawct = [[S.untwist(O(l), int(m), lift=j % 3) for j, (l, m) in enumerate(zip(p, C.q))] for p in ct]
        assert (U([S.modswitch(c, p, raw=True) for p in rawct]) == want).all()
        for p, rp, wp in zip(ct, rawct, want):
            ext = S.behz_ext(c - 1, list(O(wp)))
            assert all((x == y).all() for x, y in zip(S.drop_behz_ext(c - 1, list(O(p))), ext))
            assert all((x == y).all() for x, y in zip(S.drop_behz_ext(c - 1, rp, raw=True), ext))


@pytest.mark.parametrize("n,chain", PARAMS)
def test_sum_of_rounded_terms_and_the_evaluation_tail(n, chain):
    """the i = 0 block of eval_patstock: every term switched down on its own, then added (bin_bundle.cpp:314-324), from the exact sum of
    the kept limbs and the per-term last limbs; and the tail add_plain, add_plain, mod_switch_to_next .., clear (:345-357)"""
    C, S = context(n, chain)
    rng = np.random.default_rng(5000 + n)
    c = min(C.first, 2)
    assert c >= 1
    q = [int(m) for m in C.q[:c + 1]]
    terms = 5
    cts = [rand_ct(rng, q, n) for _ in range(terms)]
    acc0 = rand_ct(rng, q[:-1], n)
    want = O(acc0)
    for ct in cts:
        want = want + O(C.mod_switch_to_next(ct, c))
    want = U([[l % m for l, m in zip(p, q)] for p in want])
    ssum = sum(O(ct)[:, :-1] for ct in cts)
    ssum = [[l % m for l, m in zip(p, q)] for p in ssum]
    for raw in (False, True):
        s = [[S.untwist(l, m, 1) if raw else l for l, m in zip(p, q)] for p in ssum]
        v = [[S.untwist(O(ct[p][c]), q[c], 2) if raw else O(ct[p][c]) for ct in cts] for p in range(2)]
        got = [S.i0_finish(c, s[p], v[p], list(O(acc0[p])), raw=raw) for p in range(2)]
        assert (U(got) == want).all(), raw
        got = [S.i0_finish(c, s[p], v[p], None, raw=raw, store=True) for p in range(2)]
        assert (U([[(x + a) % m for x, a, m in zip(gp, ap, q)] for gp, ap in zip(got, O(acc0))]) == want).all(), raw
    # the tail
    ct, add1 = rand_ct(rng, q, n), rand_ct(rng, q, n)
    a0, mask = rng.integers(0, int(C.t), n, dtype=np.uint64), rng.integers(0, int(C.t), n, dtype=np.uint64)
    x = ct.copy()
    C.add(x, add1, c)
    C.add_plain(x, a0, c)
    C.add_plain(x, mask, c)
    for l in range(c, 0, -1):
        x = C.mod_switch_to_next(x, l)
    C.clear_irrelevant_bits(x)
    got = S.eval_epilogue(c, [list(O(p)) for p in ct], O(a0), O(mask), add1=[list(O(p)) for p in add1], clear_bits=C.irrelevant_bit_count())
    assert (U(got) == x[:, 0, :]).all()
    lifted = C.plain_lift_ntt(a0, c)
    C_l = np.stack([lifted])
    C.transform_from_ntt(C_l, c)
    assert (U(S.lift(c, O(a0))) == C_l[0]).all()
