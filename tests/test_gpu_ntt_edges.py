"""GPU tier: every transform build x modulus class at extreme inputs, bit for bit against the CPU oracle.

Modulus classes at n = 8192: narrow (50, 56), the narrow boundary (58 is narrow, 59 is wide: ntt_is_narrow), wide (59, 60), and
the 61-bit auxiliary primes behind multiply (NTT_WIDE_NEAR included).  Forms: every launch forced to 16 coefficients per lane
(APSU_HE_NTT_LATENCY_LIMBS=0), every launch forced to 8 per lane, and the default selection (switch unset), at limb counts on both
sides of each switch-over of ntt_form (apsu_amd/csrc/ntt_form.h): 256 / 257 limbs at n = 8192,
1024 / 1025 for the inverse at n = 4096.  Inputs: every residue q - 1, both operand halves at their maximum, alternating extremes,
random with extremes sprinkled in (tests/edge_values.py).
"""
import json

import numpy as np
import pytest

import apsu_amd
import edge_values as ev
from oracle import ref

pytestmark = pytest.mark.gpu

FORMS = {"x16": "0", "x8": "100000000", "auto": None}
KINDS = ("q-1", "max_halves", "alternating", "sprinkled")


def extreme_batch(qs, n, polys, seed):
    """[polys][len(qs)][n]: the four fills in turn, then random polynomials with extremes sprinkled in"""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([ev.fill_poly(KINDS[i] if i < len(KINDS) else "sprinkled", qs, n, rng) for i in range(polys)]))


def check_transforms(C, G, x, lvl, what):
    """forward against the oracle, inverse of the forward back to x, and the inverse of the extremes themselves"""
    a, g = x.copy(), x.copy()
    C.transform_to_ntt(a, lvl)
    G.transform_to_ntt_inplace(g, lvl)
    assert (a == g).all(), "forward, " + what
    G.transform_from_ntt_inplace(g, lvl)
    assert (g == x).all(), "inverse of the forward, " + what
    a, g = x.copy(), x.copy()
    C.transform_from_ntt(a, lvl)
    G.transform_from_ntt_inplace(g, lvl)
    assert (a == g).all(), "inverse, " + what


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("bits", [50, 56, 58, 59, 60])
def test_ntt_extremes_across_the_form_switch_n8192(bits, form, monkeypatch):
    """one prime (one limb per polynomial): launches of 256 and 257 limbs, forward and inverse.  In the default selection a forward
    launch above 256 limbs of narrow primes takes k_ntt<13, false, 1024, 8, 8>, wide primes stay on 16 per lane"""
    if FORMS[form] is not None:
        monkeypatch.setenv("APSU_HE_NTT_LATENCY_LIMBS", FORMS[form])
    C = ref.RefContext(8192, [bits, bits], 0, 17)
    G = apsu_amd.HeContext(n=8192, coeff_modulus=C.q, plain_modulus=C.t)
    try:
        for polys in (256, 257):
            x = extreme_batch(C.q[:1], C.n, polys, bits * 1000 + polys)
            check_transforms(C, G, x, 0, "%d-bit, %d limbs, %s" % (bits, polys, form))
    finally:
        G.close()


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("bits", [50, 56, 60])
def test_ntt_extremes_across_the_inverse_switch_n4096(bits, form, monkeypatch):
    """n = 4096: the default selection takes 8 coefficients per lane for the plain inverse up to 1024 limbs, 16 above"""
    if FORMS[form] is not None:
        monkeypatch.setenv("APSU_HE_NTT_LATENCY_LIMBS", FORMS[form])
    C = ref.RefContext(4096, [bits, bits], 0, 17)
    G = apsu_amd.HeContext(n=4096, coeff_modulus=C.q, plain_modulus=C.t)
    try:
        for polys in (1024, 1025):
            x = extreme_batch(C.q[:1], C.n, polys, bits * 1000 + polys)
            check_transforms(C, G, x, 0, "%d-bit, %d limbs, %s" % (bits, polys, form))
    finally:
        G.close()


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("bits", [50, 56, 58, 59, 60])
def test_multiply_square_relinearize_at_extremes(bits, form, monkeypatch):
    """every operand limb q - 1 (then max-halves, alternating): the BEHZ extension into the 61-bit base, the tensor loader's lazy
    input, the gathered key-switch transform (with and without its reduction on load) and the mod-down, per modulus class"""
    if FORMS[form] is not None:
        monkeypatch.setenv("APSU_HE_NTT_LATENCY_LIMBS", FORMS[form])
    C = ref.RefContext(8192, [bits, bits, bits], 0, 17)
    G = apsu_amd.HeContext(n=8192, coeff_modulus=C.q, plain_modulus=C.t)
    rng = np.random.default_rng(bits)
    try:
        rkh = np.stack([np.stack([ev.fill_poly("sprinkled", C.q, C.n, rng) for _ in range(2)]) for _ in range(C.K - 1)])
        rkx = np.stack([np.stack([ev.fill_poly("q-1", C.q, C.n) for _ in range(2)]) for _ in range(C.K - 1)])
        rk, rkxg = G.upload_relin_keys(rkh), G.upload_relin_keys(rkx)
        for lvl in range(C.first, -1, -1):
            qs = C.q[:lvl + 1]
            for kind in ("q-1", "max_halves", "alternating"):
                a = ev.fill_ct(kind, qs, C.n, 2, rng)
                b = ev.fill_ct("q-1", qs, C.n, 2, rng)
                what = "%d-bit, level %d, %s, %s" % (bits, lvl, kind, form)
                assert (C.multiply(a, b, lvl) == G.multiply(a, b, lvl)).all(), "multiply, " + what
                assert (C.square(a, lvl) == G.square(a, lvl)).all(), "square, " + what
                ct3 = ev.fill_ct(kind, qs, C.n, 3, rng)
                assert (C.relinearize(ct3, rkh, lvl) == G.relinearize(ct3, rk, lvl)).all(), "relinearize, " + what
                assert (C.relinearize(ct3, rkx, lvl) == G.relinearize(ct3, rkxg, lvl)).all(), "relinearize (keys q - 1), " + what
    finally:
        G.close()


def gather_json(bits, nb):
    ipb = 8192 // 6
    return json.dumps({
        "table_params": {"hash_func_count": 3, "table_size": ipb * nb, "max_items_per_bin": 4},
        "item_params": {"felts_per_item": 6},
        "query_params": {"ps_low_degree": 0, "query_powers": [1, 2]},
        "seal_params": {"plain_modulus_bits": 17, "poly_modulus_degree": 8192, "coeff_modulus_bits": [bits, bits, bits]},
    })


@pytest.mark.parametrize("bits", [59, 60])
def test_gathered_transform_above_256_limbs_wide_primes(bits, monkeypatch):
    """compute_powers over 24 bundle indices with two products per index at depth 1 (3 = 1 + 2, 4 = 2 + 2): one relinearisation launch
    gathers 24 * 2 * (L + 1) * L = 288 limbs, above 256, so the default selection takes k_ntt_gather<13, 1024, 8, 8> with wide
    (NTT_WIDE) targets.  Sources whose coefficients are all q - 1 / max-halves / alternating; every power against the oracle"""
    monkeypatch.delenv("APSU_HE_NTT_LATENCY_LIMBS", raising=False)
    nb = 24
    js = gather_json(bits, nb)
    p = ref.load_params(js)
    C = ref.RefContext.from_params(p)
    targets = ref.create_powers_set(0, p["max_items_per_bin"])
    depth, nodes = ref.powers_dag(p["query_powers"], targets)
    assert depth == 1 and sum(1 for nd in nodes if nd[1] == 1) == 2
    assert nb * 2 * (C.first + 2) * (C.first + 1) > 256
    rng = np.random.default_rng(bits)
    qs = C.q[:C.first + 1]
    srcs = []
    for b in range(nb):
        kinds = (KINDS[b % len(KINDS)], KINDS[(b + 1) % len(KINDS)])
        srcs.append({1: ev.fill_ct(kinds[0], qs, C.n, 2, rng), 2: ev.fill_ct(kinds[1], qs, C.n, 2, rng)})
    rkh = np.stack([np.stack([ev.fill_poly("sprinkled", C.q, C.n, rng) for _ in range(2)]) for _ in range(C.K - 1)])
    ref.set_threads(16)
    try:
        opw = [C.compute_powers(srcs[b], nodes, rkh, 0) for b in range(nb)]
    finally:
        ref.set_threads(1)
    G = apsu_amd.HeContext(js)
    try:
        rk = G.upload_relin_keys(rkh)
        pw = G.compute_powers(list(range(nb)), [[srcs[b][1], srcs[b][2]] for b in range(nb)], rk)
        for b in range(nb):
            for e in targets:
                ct, _, _ = pw.download(b, e)
                assert (ct == opw[b][e]).all(), "%d-bit, bundle index %d, power %d" % (bits, b, e)
    finally:
        G.close()
