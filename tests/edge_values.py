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


def fill_below(kind, bound, n):
    """one limb of n words below `bound`, which need not be a modulus (the unreduced gather's max_src, tests/ntt_step_model.py):
    max: every word bound - 1;  alternating: bound - 1 and 0 in turn;  sprinkled: random below bound with bound - 1 sprinkled in"""
    top = int(bound) - 1
    if kind == "max":
        return np.full(n, top, dtype=np.uint64)
    if kind == "alternating":
        out = np.zeros(n, dtype=np.uint64)
        out[::2] = top
        return out
    if kind == "sprinkled":
        rng = np.random.default_rng([n, int(bound) % 65521])
        out = rng.integers(0, int(bound), n, dtype=np.uint64)
        out[rng.random(n) < 0.25] = top
        out[:2] = (top, 0)
        return out
    raise ValueError(kind)


def fill_poly(kind, qs, n, rng=None):
    """[len(qs)][n]: limb j filled with `kind` modulo qs[j]"""
    return np.stack([fill(kind, q, n, rng) for q in qs])


def fill_ct(kind, qs, n, polys=2, rng=None):
    """[polys][len(qs)][n]"""
    return np.stack([fill_poly(kind, qs, n, rng) for _ in range(polys)])


# ---- operands of the element-wise kernels between the transforms (tests/test_gpu_kernel_steps.py)
LAYOUTS = ("same", "rotated", "max_one", "sprinkled")
PLAN_K_FIRST_INVERSE = {14: 4, 13: 4, 12: 3, 11: 2, 10: 4, 8: 2, 6: 3}      # stages of the first inverse pass (ntt_core.h plan_k)


def raw_bound(m, logn):
    """what an inverse transform that leaves out its twist can hand on (device.h, the RAW contract): below this.  A wide modulus keeps its
    values in 64 bits by conditional subtraction alone; a narrow one runs without range control from the tensor fold's last word"""
    m = int(m)
    if m * (4 * logn + 1) >= 1 << 64:
        return 1 << 64
    k = m.bit_length()
    c = (1 << k) - m
    b0 = 5 + (((c << 32) + 4 * c * c) >> (k - 1))                           # ntt_lazy_bound_q
    K = PLAN_K_FIRST_INVERSE.get(logn, 0)
    # (the first pass ends below max(2^K b0, 2 b0 + 4 (K - 1)) m; with b0 >= 5 that is 2^K b0)
    return min(1 << 64, (max(b0 << K, 2 * b0 + 4 * (K - 1)) + 4 * (logn - K)) * m)


def canonical_edges(m, extra=()):
    """extremes(m), the 32-bit boundary (the Montgomery word and the 32-bit multiplies), the residues around half, and `extra`"""
    m = int(m)
    h = (m - 1) // 2
    low_ones = ((m - 1) >> 32 << 32) | 0xFFFFFFFF
    if low_ones >= m:
        low_ones -= 1 << 32
    vals = extremes(m) + [(1 << 32) - 1, 1 << 32, low_ones, h - 1, h, h + 1, h + 2] + [int(v) for v in extra]
    out = []
    for v in vals:
        if 0 <= v < m and v not in out:
            out.append(v)
    return out


def raw_edges(m, logn, extra=()):
    """canonical_edges, the multiples of m the lazy ranges name, the transform's own bound, and the top of the 64-bit range: a RAW
    operand is any word"""
    m = int(m)
    vals = canonical_edges(m, extra) + [m, m + 1, 2 * m - 1, 2 * m, 4 * m - 1, raw_bound(m, logn) - 1, 1 << 63, (1 << 64) - m, (1 << 64) - 1]
    out = []
    for v in vals:
        if 0 <= v < 1 << 64 and v not in out:
            out.append(v)
    return out


def drop_edges(q_last):
    """last-limb residues for which (last + half) mod q_last lands on 0, q_last - 1 and just on either side of the wrap"""
    q_last = int(q_last)
    half = q_last >> 1
    return [(tgt - half) % q_last for tgt in (0, 1, q_last - 1, q_last - 2)]


def edge_limbs(layout, mods, n, rng, raw_logn=None, extra=None):
    """[len(mods)][n] words: limb j from the edge list of mods[j] (raw_logn given: RAW words), laid out
    same: coefficient k gives every limb its kind k;  rotated: limb j gets kind k + j, so cross-combinations occur;
    max_one: random, one coefficient with every limb at its largest word;  sprinkled: random with edges sprinkled in.
    extra: per limb further residues for the edge list (None or a list per limb)"""
    out = np.empty((len(mods), n), dtype=np.uint64)
    for j, m in enumerate(mods):
        m = int(m)
        ex = extra[j] if extra is not None and extra[j] is not None else ()
        kinds = np.array(raw_edges(m, raw_logn, ex) if raw_logn is not None else canonical_edges(m, ex), dtype=np.uint64)
        top = (1 << 64) - 1 if raw_logn is not None else m - 1
        if layout == "same":
            out[j] = kinds[np.arange(n) % len(kinds)]
        elif layout == "rotated":
            out[j] = kinds[(np.arange(n) + j) % len(kinds)]
        elif layout == "max_one":
            out[j] = rng.integers(0, m, n, dtype=np.uint64)
            out[j, n // 2] = top
        elif layout == "sprinkled":
            out[j] = rng.integers(0, m, n, dtype=np.uint64)
            pos = rng.random(n) < 0.25
            out[j, pos] = kinds[rng.integers(0, len(kinds), int(pos.sum()))]
        else:
            raise ValueError(layout)
    return out


def edge_block(shape, layout, mods, n, rng, raw_logn=None, extra=None):
    """shape + [len(mods)][n]: independent draws of edge_limbs (the fixed layouts shifted by one kind per block, so blocks differ)"""
    count = int(np.prod(shape)) if len(shape) else 1
    blocks = []
    for i in range(count):
        b = edge_limbs(layout, mods, n, rng, raw_logn, extra)
        blocks.append(np.roll(b, i, axis=1) if layout in ("same", "rotated") else b)
    return np.ascontiguousarray(np.stack(blocks).reshape(tuple(shape) + (len(mods), n)))


def source_with_ntt_image(C, lvl, V):
    """coefficient-form polynomials whose forward transform at chain index lvl is exactly V ([polys][lvl+1][n] canonical residues)"""
    V = np.ascontiguousarray(V, dtype=np.uint64)
    assert V.shape[1:] == (lvl + 1, C.n)
    x = V.copy()
    C.transform_from_ntt(x, lvl)
    return x
