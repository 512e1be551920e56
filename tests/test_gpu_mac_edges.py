"""GPU tier: k_mac, the BinBundle multiply-accumulate, at its worst case, bit for bit against the CPU oracle.

k_mac sums the products of s-bit operand halves without carries and folds every `chunk` terms (engine.cpp, DevLevel::mac_chunk
and mac_chunk_k; the fold count in mac_core.h).  Uniform random operands reach a quarter to a half of that bound; here every
NTT-form operand the kernel reads is an extreme (both halves at their maximum, q - 1, alternating extremes), and the chains
straddle each width's chunk.

Route through the public API: three coefficient primes put both power levels at the first data level (chain index 1), so
no source is mod-switched before its transform; with ps_low_degree = 0 and query_powers = 1..D every power is a source whose
NTT image is whatever the test picked (edge_values.source_with_ntt_image), and a BinBundle of degree d is one chain of d terms.
"""
import functools
import json

import numpy as np
import pytest

import apsu_amd
import edge_values as ev
from oracle import ref

pytestmark = pytest.mark.gpu

LONG_CHAIN = 200                      # widths whose chunk is thousands of terms: one long chain
POWER_FILLS = ("max_halves", "q-1", "alternating")      # per bundle index: the powers' NTT images ...
COEFF_FILLS = ("max_halves", "q-1", "sprinkled")        # ... and the BinBundles' stored coefficients


def mac_json(n, bits, D, bundle_indices, plain_bits):
    felts = 6 if plain_bits == 17 else 7                # item_bit_count in [80, 128]
    ipb = n // felts
    return json.dumps({
        "table_params": {"hash_func_count": 3, "table_size": ipb * bundle_indices, "max_items_per_bin": D},
        "item_params": {"felts_per_item": felts},
        "query_params": {"ps_low_degree": 0, "query_powers": list(range(1, D + 1))},
        "seal_params": {"plain_modulus_bits": plain_bits, "poly_modulus_degree": n, "coeff_modulus_bits": list(bits)},
    })


def chain_lengths(qs):
    """chunk - 2 ... chunk + 2 and 2 chunk + 1 around the two-product and the three-product chunk of the narrowest-chunk limb"""
    out = set()
    for c in (min(ev.mac_chunk(q) for q in qs), min(ev.mac_chunk_kara(q) for q in qs)):
        if 0 < c <= 130:
            out |= {c - 2, c - 1, c, c + 1, c + 2, 2 * c + 1}
    return sorted(v for v in out if v >= 1) or [LONG_CHAIN]


class Case:
    pass


def build_case(n, bits, plain_bits, per_index, power_fills, coeff_fills, seed):
    """per_index[b]: the BinBundle degrees of bundle index b; power / coeff fills per bundle index"""
    nb = len(per_index)
    D = max(max(d) for d in per_index)
    S = Case()
    S.json = mac_json(n, bits, D, nb, plain_bits)
    p = ref.load_params(S.json)
    C = ref.RefContext.from_params(p)
    assert C.first == 1 and p["bundle_idx_count"] == nb
    S.C, S.D, S.nb = C, D, nb
    qs = C.q[:2]
    rng = np.random.default_rng(seed)
    S.V, S.src, S.bundles = [], [], []

    def shared(kind, count, make):
        # constant fills are one array shared by every power / coefficient; the others rotate or cycle through a small pool
        if kind in ("max_halves", "q-1"):
            one = make(0)
            return [one] * count
        pool = [make(i) for i in range(min(count, 11))]
        return [pool[i % len(pool)] for i in range(count)]

    for b in range(nb):
        base = np.stack([ev.fill_poly(power_fills[b], qs, n, rng) for _ in range(2)])
        imgs = shared(power_fills[b], D, lambda i: np.ascontiguousarray(np.roll(base, i, axis=2)))
        srcs = {id(a): ev.source_with_ntt_image(C, 1, a) for a in imgs}
        V = {e: imgs[e - 1] for e in range(1, D + 1)}
        S.V.append(V)
        S.src.append([srcs[id(imgs[e - 1])] for e in range(1, D + 1)])
        plist = [None] + [V[e] for e in range(1, D + 1)]
        pool = shared(coeff_fills[b], 11, lambda i: ev.fill_poly(coeff_fills[b], qs, n, rng))
        for ci, deg in enumerate(per_index[b]):
            coeffs = [rng.integers(0, C.t, n, dtype=np.uint64)] + [pool[(ci + i) % len(pool)] for i in range(deg)]
            flags = [False] + [True] * deg
            mask = C.encode(rng.integers(0, C.t, n, dtype=np.uint64))
            exp = C.eval(plist, coeffs, 1, mask)
            S.bundles.append(dict(b=b, ci=ci, deg=deg, coeffs=coeffs, flags=flags, mask=mask, exp=exp))
    S.rk = np.stack([np.stack([np.stack([rng.integers(0, q, n, dtype=np.uint64) for q in C.q]) for _ in range(2)])
                     for _ in range(C.K - 1)])
    return S


def run_case(S, monkeypatch, kara, packed):
    monkeypatch.setenv("APSU_HE_MAC_KARA", str(kara))
    monkeypatch.setenv("APSU_HE_PACKED_ROWS", str(packed))
    G = apsu_amd.HeContext(S.json)
    try:
        assert G.q == S.C.q and G.first_chain_idx == 1
        rk = G.upload_relin_keys(S.rk)
        pw = G.compute_powers(list(range(S.nb)), S.src, rk)
        for b in range(S.nb):                             # the powers k_mac reads are exactly the chosen images
            for e in (1, S.D):
                ct, ci, is_ntt = pw.download(b, e)
                assert ci == 1 and is_ntt and (ct == S.V[b][e]).all(), "power %d of bundle index %d" % (e, b)
        gb = [G.upload_bundle(x["b"], x["ci"], x["coeffs"], x["flags"]) for x in S.bundles]
        out = G.eval_bundles(gb, pw, rk, [x["mask"] for x in S.bundles])
        for i, x in enumerate(S.bundles):
            assert (out[i][:2] == x["exp"]).all(), "bundle index %d, chain of %d terms (KARA=%d, packed=%d)" % (x["b"], x["deg"], kara, packed)
    finally:
        G.close()


WIDTHS = [24, 30, 32, 48, 49, 50, 52, 56, 57, 58, 59, 60]


@functools.lru_cache(maxsize=1)
def width_case(bits):
    C0 = ref.RefContext(8192, [bits] * 3, 0, 17)
    lengths = chain_lengths(C0.q[:2])
    per_index = [lengths] * len(POWER_FILLS)
    return build_case(8192, [bits] * 3, 17, per_index, POWER_FILLS, COEFF_FILLS, seed=bits)


@pytest.mark.parametrize("bits,kara,packed", [(b, k, p) for b in WIDTHS for k in (0, 1) for p in (0, 1)])   # one width at a time (cache)
def test_mac_worst_case_chains_every_width(bits, kara, packed, monkeypatch):
    """n = 8192, three `bits`-bit primes: chains around each chunk (or one long chain), every operand an extreme"""
    S = width_case(bits)
    if kara and not all(ev.mac_chunk_kara(q) for q in S.C.q[:2]):
        assert bits >= 59                                 # (the three-product form is not usable there: KARA=1 is the KARA=0 run)
    run_case(S, monkeypatch, kara, packed)


def test_mac_chunk_rule_matches_the_widths():
    """the chain lengths above do straddle a mid-chain fold for the 56..60-bit widths (2 chunk + 1 folds twice)"""
    assert chain_lengths(ref.RefContext(8192, [60] * 3, 0, 17).q[:2]) == [5, 6, 7, 8, 9, 15]
    C = ref.RefContext(8192, [58] * 3, 0, 17)
    assert ev.mac_chunk(C.q[0]) == 31 and ev.mac_chunk_kara(C.q[0]) == 15
    assert 63 in chain_lengths(C.q[:2]) and 31 in chain_lengths(C.q[:2])
    C = ref.RefContext(8192, [56] * 3, 0, 17)
    assert ev.mac_chunk(C.q[0]) == 127 and 255 in chain_lengths(C.q[:2])
    assert chain_lengths(ref.RefContext(8192, [52] * 3, 0, 17).q[:2]) == [LONG_CHAIN]


@pytest.mark.parametrize("n,bits,deg", [(2048, [18, 18, 18], 9), (8192, [60, 60, 60], 15), (8192, [56, 56, 56], 65)])
@pytest.mark.parametrize("kara", [0, 1])
def test_mac_stream_aliasing(n, bits, deg, kara, monkeypatch):
    """1, 3, 4, 5 and 9 BinBundles of one degree per bundle index: k_mac takes G = 4 streams per job and lets the missing streams of
    a short job alias a real one; every BinBundle holds different extremes, so an aliased read or write shows"""
    counts = [1, 3, 4, 5, 9]
    plain_bits = 14 if n == 2048 else 17
    fills_p = tuple(("max_halves", "q-1", "alternating", "max_halves", "q-1")[: len(counts)])
    fills_c = ("sprinkled",) * len(counts)                 # every BinBundle of an index different
    S = build_case(n, bits, plain_bits, [[deg] * c for c in counts], fills_p, fills_c, seed=n + deg)
    run_case(S, monkeypatch, kara, 1)
    run_case(S, monkeypatch, kara, 0)
