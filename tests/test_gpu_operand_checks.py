"""GPU tier: tier-1 calls refuse caller ciphertext data that is not canonical, and contexts refuse coefficient primes wider than
60 bits (SEAL_USER_MOD_BIT_COUNT_MAX), both with ValueError and never with a silently wrong limb or a device error.

The kernels take canonical residues: the product-free inverse butterflies wrap mod 2^64 on a word >= q, the lazy loaders bound
their sums by q.  A word in [q, 2q) or near 2^64 in any limb of any operand is refused (seal::is_data_valid_for), the way the query
path's check_residues refuses a query ciphertext."""
import json

import numpy as np
import pytest

import apsu_amd
import edge_values as ev
from oracle import ref

pytestmark = pytest.mark.gpu


def bad_words(q):
    return [q, q + 1, 2 * q - 1, (1 << 64) - 1, (1 << 64) - q]


@pytest.mark.parametrize("n,bits", [(4096, [36, 36, 36]), (8192, [56, 56, 50]), (8192, [60, 60, 60])])
def test_tier1_refuses_non_canonical_words(n, bits):
    C = ref.RefContext(n, bits, 0, 17)
    G = apsu_amd.HeContext(n=n, coeff_modulus=C.q, plain_modulus=C.t)
    rng = np.random.default_rng(n + bits[0])
    rkh = np.stack([np.stack([ev.fill_poly("sprinkled", C.q, C.n, rng) for _ in range(2)]) for _ in range(C.K - 1)])
    rk = G.upload_relin_keys(rkh)
    lvl = C.first
    qs = C.q[:lvl + 1]
    pt = rng.integers(0, C.t, C.n, dtype=np.uint64)
    pt_ntt = C.plain_lift_ntt(pt, lvl)

    def calls(x2, x3, ptn):
        good2 = ev.fill_ct("sprinkled", qs, C.n, 2, rng)
        return {
            "transform_to_ntt": lambda: G.transform_to_ntt_inplace(x2.copy(), lvl),
            "transform_from_ntt": lambda: G.transform_from_ntt_inplace(x2.copy(), lvl),
            "multiply_plain_ntt": lambda: G.multiply_plain_ntt(x2, ptn, lvl),
            "multiply_plain": lambda: G.multiply_plain(x2, pt, lvl),
            "add (acc)": lambda: G.add_inplace(x2.copy(), good2, lvl),
            "add (x)": lambda: G.add_inplace(good2.copy(), x2, lvl),
            "add_plain": lambda: G.add_plain_inplace(x2.copy(), pt, lvl),
            "multiply (a)": lambda: G.multiply(x2, good2, lvl),
            "multiply (b)": lambda: G.multiply(good2, x2, lvl),
            "square": lambda: G.square(x2, lvl),
            "multiply_sized": lambda: G.multiply_sized(x2, good2, lvl),
            "relinearize": lambda: G.relinearize(x3, rk, lvl),
            "mod_switch_to_next": lambda: G.mod_switch_to_next(x2, lvl),
        }

    try:
        for poly in (0, 1):
            for j, q in enumerate(qs):
                for w in bad_words(int(q)):
                    x2 = ev.fill_ct("sprinkled", qs, C.n, 2, rng)
                    x3 = ev.fill_ct("sprinkled", qs, C.n, 3, rng)
                    k = int(rng.integers(0, C.n))
                    x2[poly, j, k] = np.uint64(w)
                    x3[2 - poly, j, k] = np.uint64(w)
                    ptn = pt_ntt.copy()
                    if poly == 0:
                        ptn[j, k] = np.uint64(w)
                    for name, fn in calls(x2, x3, pt_ntt).items():
                        if name == "add_plain" and poly == 1:
                            continue                      # add_plain reads (and writes) c0 only
                        with pytest.raises(ValueError, match="outside"):
                            fn()
                    if poly == 0:                                 # the plaintext operand of multiply_plain_ntt alone
                        with pytest.raises(ValueError):
                            G.multiply_plain_ntt(ev.fill_ct("sprinkled", qs, C.n, 2, rng), ptn, lvl)
        # the context still works, and canonical extremes pass (q - 1 everywhere)
        x = ev.fill_ct("q-1", qs, C.n, 2)
        a, g = x.copy(), x.copy()
        C.transform_from_ntt(a, lvl)
        G.transform_from_ntt_inplace(g, lvl)
        assert (a == g).all()
        assert (C.multiply(x, x.copy(), lvl) == G.multiply(x, x.copy(), lvl)).all()
    finally:
        G.close()


def test_coefficient_primes_above_60_bits_are_refused():
    """60-bit primes are accepted (and exact: tests/test_gpu_ntt_edges.py, test_gpu_mac_edges.py); a 61-bit prime is refused through
    the explicit-modulus constructor and 61 coefficient bits through the JSON one"""
    n = 8192
    C = ref.RefContext(n, [60, 60], 0, 17)
    G = apsu_amd.HeContext(n=n, coeff_modulus=C.q, plain_modulus=C.t)
    G.close()
    q61 = ((1 << 61) - 1) // (2 * n) * (2 * n) + 1
    while not all(pow(w, q61 - 1, q61) == 1 for w in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)):
        q61 -= 2 * n
    assert q61.bit_length() == 61
    with pytest.raises(ValueError):
        apsu_amd.HeContext(n=n, coeff_modulus=[q61, C.q[1]], plain_modulus=C.t)
    with pytest.raises(ValueError):
        apsu_amd.HeContext(n=n, coeff_modulus=[C.q[0], q61], plain_modulus=C.t)
    js = {"table_params": {"hash_func_count": 3, "table_size": n // 6, "max_items_per_bin": 4},
          "item_params": {"felts_per_item": 6}, "query_params": {"ps_low_degree": 0, "query_powers": [1, 2]},
          "seal_params": {"plain_modulus_bits": 17, "poly_modulus_degree": n, "coeff_modulus_bits": [60, 60, 60]}}
    apsu_amd.HeContext(json.dumps(js)).close()
    js["seal_params"]["coeff_modulus_bits"] = [61, 60, 60]
    with pytest.raises(ValueError):
        apsu_amd.HeContext(json.dumps(js))
