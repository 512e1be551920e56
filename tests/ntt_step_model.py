"""The transform steps of apsu_he_debug_run_step (ntt, ntt_gather, intt_tensor; apsu_amd/csrc/engine_ntt_steps.cpp) on Python integers,
the range statements the kernels rest on, a solver for the tensor loader's worst operands, and the table of launches the GPU test
issues (a plain helper module: tests/test_ntt_step_model_cpu.py holds it to the definition, the C oracle and the CPU emulation,
tests/test_gpu_ntt_steps.py holds the kernels to it).

  forward   out[i] = a(psi^(2 brv(i) + 1)) mod m, psi the minimal primitive 2n-th root (oracle/pymodel.py), by butterflies
  inverse   its inverse, n^-1 included
  RAW       a word w at coefficient k of an inverse transform that left out its twist stands for w n^-1 psi^-k mod m
  gather    the forward transform of the source words reduced mod the target
  tensor    a0 b0, a0 b1 + a1 b0, a1 b1 mod m in front of the inverse

Everything is exact; numpy object arrays only carry the Python integers through the stages.
"""
import numpy as np

from oracle import pymodel

W64 = 1 << 64
MAP_RAW = 1 << 30
SPLIT_LOGN = 15
LATENCY_AUTO = None                                  # APSU_HE_NTT_LATENCY_LIMBS unset
AUTO_LIMBS = W64 - 1                                 # NTT_FORM_AUTO as emu_ntt_form takes it
KIND = {"forward": 0, "inverse": 1, "gather": 2, "tensor": 3}


def O(x):
    return np.array([int(v) for v in np.asarray(x).reshape(-1)], dtype=object).reshape(np.asarray(x).shape)


def U(x):
    return np.array([int(v) for v in np.asarray(x, dtype=object).reshape(-1)], dtype=np.uint64).reshape(np.asarray(x, dtype=object).shape)


# ---------------------------------------------------------------------------------------------------------------- the transforms
_ROOTS = {}


def roots(m, logn):
    """(psi, [psi^brv(k, logn) for k < n]) for modulus m"""
    if (m, logn) not in _ROOTS:
        n = 1 << logn
        psi = pymodel.minimal_primitive_root(2 * n, m)
        pw = [1] * n
        for e in range(1, n):
            pw[e] = pw[e - 1] * psi % m
        _ROOTS[(m, logn)] = (psi, np.array([pw[pymodel.brv(k, logn)] for k in range(n)], dtype=object))
    return _ROOTS[(m, logn)]


def forward(a, m, logn):
    """natural order in, out[i] = a(psi^(2 brv(i) + 1)): Cooley-Tukey, stage with 2^s blocks multiplies block b's lower half by psi^brv(2^s + b)"""
    n = 1 << logn
    w = roots(m, logn)[1]
    x = O(a) % m
    blocks, half = 1, n >> 1
    while blocks < n:
        x = x.reshape(blocks, 2, half)
        v = x[:, 1, :] * w[blocks:2 * blocks].reshape(blocks, 1) % m
        x = np.stack([(x[:, 0, :] + v) % m, (x[:, 0, :] - v) % m], axis=1)
        blocks, half = blocks * 2, half >> 1
    return x.reshape(n)


def inverse(A, m, logn):
    """the inverse of forward(): the stages undone last to first, the halvings collected into n^-1"""
    n = 1 << logn
    w = roots(m, logn)[1]
    x = O(A) % m
    blocks, half = n >> 1, 1
    while blocks >= 1:
        x = x.reshape(blocks, 2, half)
        winv = np.array([pow(int(v), -1, m) for v in w[blocks:2 * blocks]], dtype=object).reshape(blocks, 1)
        x = np.stack([(x[:, 0, :] + x[:, 1, :]) % m, (x[:, 0, :] - x[:, 1, :]) * winv % m], axis=1)
        blocks, half = blocks >> 1, half * 2
    return x.reshape(n) * pow(n, -1, m) % m


def evaluate_at(a, m, logn, i):
    """the definition at ONE output index: Horner at psi^(2 brv(i) + 1)"""
    psi = roots(m, logn)[0]
    x = pow(psi, 2 * pymodel.brv(i, logn) + 1, m)
    acc = 0
    for c in reversed([int(v) for v in a]):
        acc = (acc * x + c) % m
    return acc


def raw_residue(words, m, logn):
    """what RAW words stand for: w n^-1 psi^-k mod m at coefficient k"""
    n = 1 << logn
    psi = roots(m, logn)[0]
    ipsi = pow(psi, -1, m)
    tw, cur = [0] * n, pow(n, -1, m)
    for k in range(n):
        tw[k] = cur
        cur = cur * ipsi % m
    return O(words) * np.array(tw, dtype=object) % m


def gather(src, m, logn):
    return forward(O(src) % m, m, logn)


def tensor_products(a0, a1, b0, b1, m):
    a0, a1, b0, b1 = O(a0), O(a1), O(b0), O(b1)
    return [a0 * b0 % m, (a0 * b1 + a1 * b0) % m, a1 * b1 % m]


def intt_tensor(a0, a1, b0, b1, m, logn):
    return [inverse(p, m, logn) for p in tensor_products(a0, a1, b0, b1, m)]


# ---------------------------------------------------------------------------------------------------------------- ranges (ntt_core.h)
PLAN = {14: (3, 3, 4, 4), 13: (3, 3, 3, 4), 12: (3, 3, 3, 3), 11: (3, 3, 3, 2), 10: (3, 3, 4), 8: (3, 3, 2), 6: (3, 3)}   # plan_k, 16 per lane
PLAN8 = {13: (2, 3, 3, 3, 2), 12: (3, 3, 3, 3)}                                                                          # 8 per lane


def stages(logn):
    """the stages one workgroup runs, which is what the tables' `narrow` is computed for: the halves of the split transform at n = 32768"""
    return logn - 1 if logn == SPLIT_LOGN else logn


def is_narrow(m, logn):
    return m * (4 * logn + 1) < W64


def gather_nored_ok(m, max_src, logn):
    return is_narrow(m, logn) and m * 4 * logn + max_src <= W64


def fold_params(m):
    """(k, c) of m = 2^k - c where ntt_reduce_any folds, else (0, 0)"""
    k = m.bit_length()
    c = (1 << k) - m
    if k < 33 or k > 62 or c >> 32 or ((1 << (64 - k)) + 2) * c > 1 << k:
        return 0, 0
    return k, c


def fold128_ok(m):
    k, c = fold_params(m)
    return 44 <= k <= 61 and c < 1 << 24


def mod_class(m, logn):
    """narrow / wide_near / wide: the range discipline a limb's workgroup takes"""
    if is_narrow(m, stages(logn)):
        return "narrow"
    return "wide_near" if m < 1 << 61 and 4 * m < 1 << 63 and ((1 << 63) - 4 * m) < 1 << 32 else "wide"


def reduce128_lazy(P, m):
    """ntt_reduce128_lazy: the fold's last word as a function of the 128-bit sum P"""
    k, c = fold_params(m)
    s = k - 32
    pl = P & ((1 << k) - 1)
    ph = (P >> k) & (W64 - 1)
    a = (ph & 0xFFFFFFFF) * c
    t = ((ph >> 32) & 0xFFFFFFFF) * c
    w = pl + a + ((t >> s) & 0xFFFFFFFF) * c + ((t & ((1 << s) - 1)) << 32)
    assert w < W64
    return w


def lazy_bound_q(m):
    k, c = fold_params(m)
    return 5 + (((c << 32) + 4 * c * c) >> (k - 1))


def lazy_input_ok(m, logn):
    if not fold128_ok(m):
        return False
    if not is_narrow(m, logn):
        return True
    K = PLAN[logn][-1]
    return m * ((lazy_bound_q(m) << K) + 4 * (logn - K)) < W64


def raw_bound(m, logn, lazy_source=False):
    """device.h, the RAW contract: a wide modulus leaves any 64-bit word; a narrow one words below
    (max(2^K b0, 2 b0 + 4 (K - 1)) + 4 (logn - K)) m, K the stages of the first inverse pass, b0 = 1 for a canonical source or
    ntt_lazy_bound_q for the tensor fold's last word.  The walk over the first pass: stage 1 has only product-free butterflies (2 b0); a
    later stage doubles a product-free chain and adds 4 to everything else, so after K stages the largest word is a chain that stayed
    product-free (2^K b0) or one that left it after stage 1 (2 b0 + 4 (K - 1)); every stage of the other passes adds 4."""
    if not is_narrow(m, logn):
        return W64
    K = PLAN[logn][-1]
    b0 = lazy_bound_q(m) if lazy_source and lazy_input_ok(m, logn) else 1
    return (max(b0 << K, 2 * b0 + 4 * (K - 1)) + 4 * (logn - K)) * m


# ---------------------------------------------------------------------------------------------------------------- the worst operands
def fold_word(quad, m):
    x0, y0, x1, y1 = quad
    return reduce128_lazy(x0 * y0 + x1 * y1, m)


def random_fold_max(m, draws=20000, seed=2022):
    """the largest fold word of `draws` seeded random canonical quadruples (what pseudo-random tests feed the loader)"""
    rng = np.random.default_rng([seed, m % 65521])
    v = rng.integers(0, m, (draws, 4), dtype=np.uint64)
    return max(fold_word([int(x) for x in row], m) for row in v)


def solve_lazy_operands(m, keep=4, spread=96):
    """Canonical (x0, y0, x1, y1) whose sum of products has the largest fold word found, best first.  The route: the low word of ph all
    ones (a = (2^32 - 1) c), hi32(ph) c = -1 mod 2^(k-32) so that (t mod 2^s) << 32 is maximal -- the term an all-(q-1) fill misses --
    and pl near 2^k - 1.  P = (m - 1) S - e y1 with x0 = m - 1, x1 = m - 1 - e: for every small e one y1 solves the congruence, and it is
    kept when both y fit below m; where the exact target has no such form, the nearest below it that has."""
    k, c = fold_params(m)
    assert fold128_ok(m)
    s = k - 32
    top = 2 * (m - 1) * (m - 1)
    h0 = (-pow(c, -1, 1 << s)) % (1 << s)
    found = []
    for h in (h0 + (1 << s), h0, h0 + (1 << s) - (1 << (s - 1)), h0 - 1 + (1 << s)):
        for lo in (0xFFFFFFFF, 0xFFFFFFFE):
            target = ((((h << 32) | lo) << k) | ((1 << k) - 1))
            if target > top or h < 0:
                continue
            for e in range(1, spread):
                x0, x1 = m - 1, m - 1 - e
                for back in range(0, 3):
                    P = target - back
                    # P = x0 y0 + x1 y1 = x0 S - e y1 with S = y0 + y1
                    S = -(-P // x0)
                    for _ in range(e):
                        if (x0 * S - P) % e == 0:
                            break
                        S += 1
                    else:
                        continue                      # (x0 and e share a factor that P does not have)
                    y1 = (x0 * S - P) // e
                    y0 = S - y1
                    if 0 <= y0 < m and 0 <= y1 < m:
                        assert x0 * y0 + x1 * y1 == P
                        found.append((reduce128_lazy(P, m), (x0, y0, x1, y1)))
    found.append((fold_word((m - 1,) * 4, m), (m - 1,) * 4))
    found.sort(reverse=True)
    out = []
    for w, quad in found:
        if quad not in out:
            out.append(quad)
        if len(out) == keep:
            break
    return out


# ---------------------------------------------------------------------------------------------------------------- the contexts
T_PLAIN = 65537                                       # 1 mod 2n for every ring size here, below every coefficient prime
LOGNS = (6, 8, 10, 11, 12, 13, 14, 15)
LATENCIES = {12: (LATENCY_AUTO, 0, 100000000), 13: (LATENCY_AUTO, 0, 100000000)}


def prime_below(start, n):
    v = (start - 1) // (2 * n) * (2 * n) + 1
    while not pymodel.is_prime(v):
        v -= 2 * n
    return v


def prime_above(start, n):
    v = -(-(start - 1) // (2 * n)) * (2 * n) + 1
    while v < start or not pymodel.is_prime(v):
        v += 2 * n
    return v


_PRIMES = {}


def context_primes(logn):
    """chosen, not generated: a 60-bit wide prime; the largest prime under the narrow criterion of this ring and the smallest above it
    (no fold: Barrett runs); a 50-bit prime with a large c (0x3ffffffef4001 at n = 8192); a prime below 33 bits"""
    if logn not in _PRIMES:
        n = 1 << logn
        edge = W64 // (4 * stages(logn) + 1)          # m is narrow iff m <= edge
        c50 = 0x3FFFFFFEF4001 if logn == 13 else prime_below((1 << 50) - (1 << 22), n)
        q = [prime_below(1 << 60, n), prime_below(edge + 1, n), prime_above(edge + 1, n), c50, prime_below(1 << 30, n)]
        assert is_narrow(q[1], stages(logn)) and not is_narrow(q[2], stages(logn)) and not is_narrow(q[0], stages(logn)) and q[2] < 1 << 60
        assert fold_params(q[1]) == (0, 0) and fold_params(q[2]) == (0, 0) and fold_params(q[4]) == (0, 0) and fold128_ok(q[3]) and fold128_ok(q[0])
        assert all((p - 1) % (2 * n) == 0 for p in q) and len(set(q)) == 5
        _PRIMES[logn] = q
    return _PRIMES[logn]


# ---------------------------------------------------------------------------------------------------------------- the launches
def form_rows():
    """every row of k_ntt_forms, k_ntt_gather_forms and k_intt_tensor_forms (kernels_ntt.hip) by direction, and the two stage kernels:
    (family, logn, threads, coeffs per lane, min waves, direction)"""
    rows = []
    ntt = [(14, 1024, 16, 4), (13, 1024, 8, 4), (12, 512, 8, 4), (13, 512, 16, 4), (12, 256, 16, 4), (11, 128, 16, 4), (10, 64, 16, 4), (8, 64, 16, 4), (6, 64, 16, 4)]
    for r in ntt:
        rows += [("k_ntt",) + r + ("inverse",), ("k_ntt",) + r + ("forward",)]
    rows.append(("k_ntt", 13, 1024, 8, 8, "forward"))
    for r in [(13, 1024, 8, 4), (12, 512, 8, 4), (13, 1024, 8, 8)] + [r for r in ntt if r[2] == 16]:
        rows.append(("k_ntt_gather",) + r + ("forward",))
    for r in ntt:
        rows.append(("k_intt_tensor",) + r + ("inverse",))
    rows += [("k_ntt_first_stage", 15, 0, 0, 0, "forward"), ("k_ntt_first_stage", 15, 0, 0, 0, "gather"), ("k_ntt_last_stage", 15, 0, 0, 0, "inverse")]
    return rows


def launches():
    """The launches tests/test_gpu_ntt_steps.py issues, one dict per launch shape: logn, kind (forward / inverse / gather / tensor), limbs
    of the launch, latency (the context's APSU_HE_NTT_LATENCY_LIMBS: None = unset), narrow (what the step states about the map's moduli),
    and what the test puts into it: case, aux (the auxiliary base of the context), and for a tensor launch njobs x limbs + n_plain."""
    out = []

    def add(logn, kind, limbs, latency, narrow, case, aux="narrow", **kw):
        out.append(dict(logn=logn, kind=kind, limbs=limbs, latency=latency, narrow=narrow, case=case, aux=aux, **kw))

    for logn in LOGNS:
        big = logn >= 14
        nall = 5 if big else 13                       # moduli of the "all" map (a handful at the two largest rings)
        for aux in ("narrow", "seal"):
            for lat in LATENCIES.get(logn, (LATENCY_AUTO,)):
                add(logn, "forward", nall + 2, lat, False, "all", aux)
                add(logn, "inverse", 2 * nall + 1, lat, False, "all", aux)
                add(logn, "forward", 3, lat, False, "short", aux)
                add(logn, "inverse", 3, lat, False, "short", aux)
                add(logn, "gather", nall + 2, lat, False, "reduced", aux)
                if logn < SPLIT_LOGN:
                    add(logn, "gather", 5, lat, True, "nored", aux)
                    add(logn, "tensor", 3 * nall, lat, False, "operands", aux, njobs=1, tlimbs=nall, n_plain=0)
                    if aux == "narrow":
                        # pairs % 8 in {1, 7, 0} and 15 > 8; a handful of limbs at n = 16384
                        # (stride, dgap: limbs between an operand's polynomials / between two jobs' outputs, at and above limbs / 3 limbs)
                        for njobs, tl, n_plain, stride, dgap in (((1, 1, 0, 1, 3), (1, 3, 2, 5, 11)) if big else ((1, 1, 0, 1, 3), (1, 7, 3, 9, 23), (2, 4, 0, 4, 12), (3, 5, 3, 7, 17))):
                            add(logn, "tensor", 3 * njobs * tl + n_plain, lat, False, "shape", aux, njobs=njobs, tlimbs=tl, n_plain=n_plain, stride=stride, dgap=dgap)
    # the switch-overs of the default selection (ntt_form.h): 256 | 257 limbs at n = 8192, 1024 | 1025 at n = 4096
    for limbs in (256, 257):
        add(13, "forward", limbs, LATENCY_AUTO, True, "switch")
        add(13, "forward", limbs, LATENCY_AUTO, False, "switch")
        add(13, "inverse", limbs, LATENCY_AUTO, False, "switch")
    add(13, "gather", 257, LATENCY_AUTO, True, "nored-switch")
    add(13, "gather", 257, LATENCY_AUTO, False, "reduced-switch")
    for limbs in (1024, 1025):
        add(12, "forward", limbs, LATENCY_AUTO, False, "switch")
        add(12, "inverse", limbs, LATENCY_AUTO, False, "switch")
    return out


def kernels_of(row, form):
    """the form-table rows (form_rows) a launch runs, given ntt_form's answer (threads, coeffs, min_waves, split) for it"""
    threads, coeffs, minw, split = form
    kind = row["kind"]
    direction = "inverse" if kind in ("inverse", "tensor") else "forward"
    if split:
        assert kind != "tensor"
        stage = ("k_ntt_last_stage", 15, 0, 0, 0, "inverse") if kind == "inverse" else ("k_ntt_first_stage", 15, 0, 0, 0, "gather" if kind == "gather" else "forward")
        return [("k_ntt", 14, threads, coeffs, minw, direction), stage]
    family = {"forward": "k_ntt", "inverse": "k_ntt", "gather": "k_ntt_gather", "tensor": "k_intt_tensor"}[kind]
    return [(family, row["logn"], threads, coeffs, minw, direction)]


# ---------------------------------------------------------------------------------------------------------------- the directed inputs
FILLS = ("q-1", "max_halves", "alternating", "sprinkled")
NORED_FILLS = ("max", "alternating", "sprinkled")
TENSOR_LAYOUTS = ("solved", "rotated", "sprinkled", "q-1")


def canonical_fill(kind, m, n):
    import edge_values as ev
    return ev.fill(kind, m, n, np.random.default_rng([n, m % 65521, FILLS.index(kind)]))


def reduced_sources(mods, logn, layout="rotated"):
    """one source limb per modulus: 0, q - 1, q, 2q, 2^63, 2^64 - q, 2^64 - 1 and the other RAW edges of that modulus (edge_values.raw_edges)"""
    import edge_values as ev
    n = 1 << logn
    return ev.edge_limbs(layout, mods, n, np.random.default_rng([n, len(mods), 7]), raw_logn=logn)


def nored_max_src(mods, logn):
    """the boundary of ntt_gather_nored_ok for the widest target: 2^64 - 4 logn q"""
    return W64 - 4 * logn * max(mods)


def nored_source(kind, max_src, n):
    import edge_values as ev
    return ev.fill_below(kind, max_src, n)


_SOLVED = {}


def tensor_quads(m):
    """the quadruples a tensor test lays out for modulus m: the solved ones where the modulus has the fold (else the range edges), then q - 1"""
    if m not in _SOLVED:
        quads = solve_lazy_operands(m) if fold128_ok(m) else [(m - 1, m - 2, m - 2, m - 1), (m - 1, (m - 1) // 2, (m + 1) // 2, m - 1)]
        _SOLVED[m] = quads + ([(m - 1,) * 4] if (m - 1,) * 4 not in quads else [])
    return _SOLVED[m]


def tensor_operands(layout, m, n, shift=0):
    """(a0, a1, b0, b1) [n] each, canonical, with the d1 = a0 b1 + a1 b0 sum taking (x0, y0, x1, y1) = (a0, b1, a1, b0) of a quadruple:
    solved: the best one at every coefficient;  rotated: coefficient k takes quadruple k + shift;  sprinkled: random with the quadruples
    sprinkled in and each of them once at the front;  q-1: every operand q - 1"""
    quads = tensor_quads(m)
    rng = np.random.default_rng([n, m % 65521, shift, 11])
    if layout == "solved":
        pick = np.zeros(n, dtype=np.int64)
    elif layout == "q-1":
        pick = np.full(n, quads.index((m - 1,) * 4), dtype=np.int64)
    elif layout == "rotated":
        pick = (np.arange(n) + shift) % len(quads)
    elif layout == "sprinkled":
        pick = np.where(rng.random(n) < 0.25, rng.integers(0, len(quads), n), -1)
        pick[:len(quads)] = np.arange(len(quads))
    else:
        raise ValueError(layout)
    Q = np.array(quads, dtype=np.uint64)
    rnd = rng.integers(0, m, (n, 4), dtype=np.uint64)
    v = np.where((pick >= 0)[:, None], Q[np.maximum(pick, 0)], rnd)
    x0, y0, x1, y1 = (np.ascontiguousarray(v[:, i]) for i in range(4))
    return x0, x1, y1, y0                               # a0, a1, b0, b1


def largest_fold_word(m, a0, a1, b0, b1):
    """the largest word ntt_reduce128_lazy hands the transform among the three products of these operand limbs"""
    a0, a1, b0, b1 = O(a0), O(a1), O(b0), O(b1)
    return max(max(reduce128_lazy(int(p), m) for p in set(P)) for P in (a0 * b0, a0 * b1 + a1 * b0, a1 * b1))
