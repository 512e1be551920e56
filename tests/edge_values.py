"""Worst-case operands for the kernels' lazy ranges (a plain helper module, imported by the edge tests).

The kernels keep values above q for several steps or sum products without carries under bounds argued per modulus; uniform
random residues sit far below those bounds.  These helpers build the operands that reach them:

  * extremes(q, s): the range edges of one residue, plus the residue whose two s-bit halves (k_mac's operand split,
    dev_consts.cpp, build_level: s = ceil(bits(q) / 2)) are both as large as a residue below q allows;
  * fill(...): whole polynomials of one extreme, of alternating extremes, or random with extremes sprinkled in;
  * source_with_ntt_image(C, lvl, V): a coefficient-form ciphertext whose forward transform is exactly V (the oracle's
    inverse transform), so a test picks the NTT-form operands a multiply-accumulate reads.
"""
import numpy as np

FILLS = ("max_halves", "q-1", "alternating", "sprinkled")


def mac_shift(q):
    """k_mac's operand split width: both halves of a residue < 2^s"""
    return (int(q).bit_length() + 1) // 2


def mac_chunk(q):
    """terms per carry-free chunk of the two-cross-product form (mac_core.h mac_chunk_of, DevLevel::mac_chunk; held to it by test_dev_consts_cpu.py and test_mac_core_cpu.py)"""
    s = mac_shift(q)
    cap = 1 << (63 - 2 * s)
    return min(cap - 1 if cap > 2 else 2, 1 << 20)


def mac_chunk_kara(q):
    """terms per chunk of the three-product form; 0 where the form is not usable for q (mac_core.h: mac_chunk_k_of where mac_kara_usable)"""
    s = mac_shift(q)
    if 62 - 2 * s < 3:
        return 0
    capk = 1 << (62 - 2 * s) if 2 * s + 2 < 64 else 0
    return min(capk - 1 if capk > 2 else 0, 1 << 20)


def max_halves(q, s=None):
    """the largest residue below q whose low s-bit half is 2^s - 1 and whose high half is as large as q allows"""
    q = int(q)
    s = mac_shift(q) if s is None else s
    lo = (1 << s) - 1
    hi = (q - 1) >> s
    v = (hi << s) | lo
    if v >= q:
        v = ((hi - 1) << s) | lo
    assert 0 <= v < q
    return v


def extremes(q, s=None):
    q = int(q)
    vals = [0, 1, q - 1, q - 2, (q - 1) // 2, (q + 1) // 2, max_halves(q, s)]
    return [v for v in vals if 0 <= v < q]


def fill(kind, q, n, rng=None, s=None):
    """one limb of n residues mod q: every residue max_halves / q-1, alternating extremes, or random with extremes sprinkled in"""
    q = int(q)
    if kind == "max_halves":
        return np.full(n, max_halves(q, s), dtype=np.uint64)
    if kind == "q-1":
        return np.full(n, q - 1, dtype=np.uint64)
    ex = np.array(extremes(q, s), dtype=np.uint64)
    if kind == "alternating":
        return np.ascontiguousarray(ex[np.arange(n) % len(ex)])
    if kind == "sprinkled":
        rng = rng if rng is not None else np.random.default_rng(q % 65521)
        out = rng.integers(0, q, n, dtype=np.uint64)
        pos = rng.random(n) < 0.25
        out[pos] = ex[rng.integers(0, len(ex), int(pos.sum()))]
        out[: len(ex)] = ex
        return out
    raise ValueError(kind)


def fill_poly(kind, qs, n, rng=None):
    """[len(qs)][n]: limb j filled with `kind` modulo qs[j]"""
    return np.stack([fill(kind, q, n, rng) for q in qs])


def fill_ct(kind, qs, n, polys=2, rng=None):
    """[polys][len(qs)][n]"""
    return np.stack([fill_poly(kind, qs, n, rng) for _ in range(polys)])


def source_with_ntt_image(C, lvl, V):
    """coefficient-form polynomials whose forward transform at chain index lvl is exactly V ([polys][lvl+1][n] canonical residues)"""
    V = np.ascontiguousarray(V, dtype=np.uint64)
    assert V.shape[1:] == (lvl + 1, C.n)
    x = V.copy()
    C.transform_from_ntt(x, lvl)
    return x
