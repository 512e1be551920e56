"""GPU tier: the engine's own narrow auxiliary BEHZ base (the default) against SEAL's 61-bit base (APSU_HE_AUX_BASE=seal, read when a
context is created).  Both give the oracle's bits -- the oracle keeps SEAL's primes -- and each other's.  The SEAL-base runs keep the
wide transform paths (NTT_WIDE_NEAR range control, stage-1-only product-free butterflies) behind multiply covered now that the
default base no longer takes them."""
import numpy as np
import pytest

import apsu_amd
import common
from oracle import ref

pytestmark = pytest.mark.gpu

FAMILIES = [
    (8192, [56, 56, 56, 50], 0, 22),        # 16M-4096
    (8192, [50, 50, 50, 38, 30], 0, 26),    # 256M-4096
    (4096, [48, 36, 25], 0, 18),            # 1M-1024-com
    (8192, [60, 60, 60], 0, 41),            # |B| = L + 1
    (16384, [58, 58, 50, 40], 0, 22),       # one 1024-thread workgroup per limb
]


def context(monkeypatch, base, *args, **kw):
    if base:
        monkeypatch.setenv("APSU_HE_AUX_BASE", base)
    else:
        monkeypatch.delenv("APSU_HE_AUX_BASE", raising=False)
    G = apsu_amd.HeContext(*args, **kw)
    monkeypatch.delenv("APSU_HE_AUX_BASE", raising=False)
    return G


def rand_ct(C, rng, polys, lvl):
    ct = np.stack([np.stack([rng.integers(0, q, C.n, dtype=np.uint64) for q in C.q[:lvl + 1]]) for _ in range(polys)])
    for j, q in enumerate(C.q[:lvl + 1]):                         # extreme residues in the first coefficients
        ct[:, j, 0] = q - 1
        ct[:, j, 1] = 0
    return ct


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: "n%d_K%d" % (f[0], len(f[1])))
def test_multiply_relinearize_either_base(fam, monkeypatch):
    n, bits, t, pb = fam
    C = ref.RefContext(n, bits, t, pb)
    G = {b: context(monkeypatch, b, n=n, coeff_modulus=C.q, plain_modulus=C.t) for b in ("seal", "")}
    rng = np.random.default_rng(58)
    rkh = np.stack([np.stack([np.stack([rng.integers(0, q, C.n, dtype=np.uint64) for q in C.q]) for _ in range(2)])
                    for _ in range(C.K - 1)])
    rk = {b: g.upload_relin_keys(rkh) for b, g in G.items()}
    for lvl in range(C.first, -1, -1):
        a, b2, ct3 = rand_ct(C, rng, 2, lvl), rand_ct(C, rng, 2, lvl), rand_ct(C, rng, 3, lvl)
        exp_m, exp_s, exp_r = C.multiply(a, b2, lvl), C.square(a, lvl), C.relinearize(ct3, rkh, lvl)
        got = {b: (g.multiply(a, b2, lvl), g.square(a, lvl), g.relinearize(ct3, rk[b], lvl)) for b, g in G.items()}
        for b in G:
            assert (got[b][0] == exp_m).all(), ("multiply", b or "narrow", lvl)
            assert (got[b][1] == exp_s).all(), ("square", b or "narrow", lvl)
            assert (got[b][2] == exp_r).all(), ("relinearize", b or "narrow", lvl)
        assert all((x == y).all() for x, y in zip(got["seal"], got[""]))
    for g in G.values():
        g.close()


def test_16m_4096_powers_and_evaluation_either_base(monkeypatch):
    """one bundle index of 16M-4096: every target power (ComputePowers) and one BinBundle evaluated (eval_patstock), under each base"""
    js = common.param_json("16M-4096")
    S = common.make_scenario(js, {0: [170]})
    opw = common.oracle_powers(S)
    exp = common.oracle_eval(S, opw, S.bundles[0])
    res = {}
    for base in ("seal", ""):
        G = context(monkeypatch, base, js)
        rk = G.upload_relin_keys(S.rk)
        pw = G.compute_powers([0], [[S.src[0][e] for e in S.sources]], rk)
        powers = {}
        for p in S.targets:
            ct, ci, is_ntt = pw.download(0, p)
            assert (ct == opw[0][p]).all(), ("power", p, base or "narrow")
            powers[p] = ct
        b = S.bundles[0]
        gb = G.upload_bundle(b["bundle_idx"], b["cache_idx"], b["coeffs"], b["flags"])
        out = G.eval_bundles([gb], pw, rk, [b["mask"]])
        assert (out[0] == exp).all(), base or "narrow"
        assert common.check_semantics(S, b, out[0])[0]
        res[base] = (powers, out[0].copy())
        G.close()
    assert all((res["seal"][0][p] == res[""][0][p]).all() for p in S.targets)
    assert (res["seal"][1] == res[""][1]).all()

