"""GPU tier: every element-wise launcher between the transforms, one launch at a time, bit for bit against the big-integer model.

apsu_he_debug_run_step puts chosen words in front of ONE launch_* call of apsu_amd/csrc/device.h with the context's own constant
blocks; tests/kernel_step_model.py states the same step on Python integers (held to the C oracle by test_kernel_step_model_cpu.py).
Inputs go exactly up to the launcher's input contract (device.h): canonical operands at the edges of their range, RAW operands over
the whole 64-bit range (tests/edge_values.py), in four layouts, plus directed cases solved with the model: the Montgomery word r at
0, 2^31 - 1, 2^31, 2^32 - 1; alpha at 0, +-1 .. +-nB, m_sk/2, m_sk/2 + 1, m_sk - 1; the rounding of every drop on either side of its
wrap; the summed kernels at their host-checked term bounds, and a refusal one past them.  No tolerance, nothing skipped.

Shapes: n = 1024 (four workgroups of EW_T) with 3 jobs, one pass of every step at n = 64 (the tail guard) with 1 job.
"""
import ctypes as C

import numpy as np
import pytest

import apsu_amd
import edge_values as ev
import kernel_step_model as ksm
from apsu_amd import engine as E
from apsu_amd.engine import STEP_ACCUMULATE, STEP_KEY, STEP_RAW, STEP_STORE
from kernel_step_model import O, U
from oracle import pymodel

pytestmark = pytest.mark.gpu

W64 = 1 << 64
T17 = {1024: pymodel.coeff_modulus_create(1024, [17])[0], 64: pymodel.coeff_modulus_create(64, [17])[0]}
T41 = {1024: pymodel.coeff_modulus_create(1024, [41])[0], 64: pymodel.coeff_modulus_create(64, [41])[0]}


def primes_from(start, count, n):
    """`count` primes = 1 mod 2n below `start`, descending"""
    out, v = [], start // (2 * n) * (2 * n) + 1
    while len(out) < count:
        if v < start and pymodel.is_prime(v):
            out.append(v)
        v -= 2 * n
    return out


# name -> (coefficient primes by bit size or as given, plain modulus, the (L, nB) of every level from the first down, aux base)
def chain_spec(name, n):
    t17, t41 = T17[n], T41[n]
    specs = {
        "60x4": ([60] * 4, t17, [(3, 3), (2, 2), (1, 1)]),
        "58x4": ([58] * 4, t17, [(3, 3), (2, 2), (1, 1)]),
        "56x4": ([56] * 4, t17, [(3, 3), (2, 2), (1, 1)]),
        "50x4-large-c": (primes_from((1 << 50) - (1 << 22), 4, n), t17, [(3, 3), (2, 2), (1, 1)]),
        "50x6": ([50] * 6, t17, [(5, 5), (4, 4), (3, 3), (2, 2), (1, 1)]),
        "48x8": ([48] * 8, t17, [(7, 7), (6, 6), (5, 5), (4, 4), (3, 3), (2, 2), (1, 1)]),
        "60x3-t41": ([60] * 3, t41, [(2, 3), (1, 2)]),
        "60-60-30": ([60, 60, 30, 60], t17, [(3, 3), (2, 2), (1, 1)]),
        "36-36-60": ([36, 36, 60, 60], t17, [(3, 3), (2, 2), (1, 1)]),
        "60x4-seal-aux": ([60] * 4, t17, [(3, 3), (2, 2), (1, 1)]),
        "60x5": ([60] * 5, t17, [(4, 4), (3, 3), (2, 2), (1, 1)]),
        "60x5-seal-aux": ([60] * 5, t17, [(4, 4), (3, 3), (2, 2), (1, 1)]),
    }
    q, t, shapes = specs[name]
    if isinstance(q[0], int) and q[0] < 64:
        q = pymodel.coeff_modulus_create(n, q)
    return q, t, shapes


class Ctx:
    def __init__(self, name, n):
        q, t, shapes = chain_spec(name, n)
        self.name, self.n, self.logn, self.t = name, n, n.bit_length() - 1, t
        self.G = apsu_amd.HeContext(n=n, coeff_modulus=q, plain_modulus=t)
        self.first = len(q) - 2
        info = [self.G.level_info(c) for c in range(self.first + 1)]
        # the dispatch is known: every level's (L, nB) is what the chain was chosen for
        assert [(i["L"], i["nB"]) for i in reversed(info)] == shapes, (name, info)
        for c, i in enumerate(info):
            assert i["q"] == q[:c + 1] and i["p"] == q[-1] and i["unrolled"] == (i["L"] == i["nB"] <= 3)
        self.S = ksm.StepModel(n, q, t, [(i["q"], i["B"], i["m_sk"]) for i in info])
        self.clear_bits = info[0]["clear_bits"]
        self.unrolled = [i["unrolled"] for i in info]

    def rng(self, *key):
        return np.random.default_rng([self.n, len(self.name)] + [int(k) for k in key])

    def run(self, step, c, ins, outs, **kw):
        self.G.debug_run_step(step, c, ins=ins, outs=outs, **kw)


_CTX = {}


@pytest.fixture(scope="module")
def ctx(monkeypatch_module):
    def get(name, n=1024):
        if (name, n) not in _CTX:
            if name.endswith("seal-aux"):
                monkeypatch_module.setenv("APSU_HE_AUX_BASE", "seal")
            try:
                _CTX[(name, n)] = Ctx(name, n)
            finally:
                monkeypatch_module.delenv("APSU_HE_AUX_BASE", raising=False)
        return _CTX[(name, n)]
    yield get
    for X in _CTX.values():
        X.G.close()
    _CTX.clear()


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


UNROLLED_CHAINS = ["60x4", "58x4", "56x4", "50x4-large-c", "60-60-30", "36-36-60"]
ALL_CHAINS = UNROLLED_CHAINS + ["50x6", "48x8", "60x3-t41"]


def levels_of(name):
    return range(len(chain_spec(name, 64)[2]))


def same(got, want, what):
    got, want = np.asarray(got), U(want).reshape(np.asarray(got).shape)
    bad = np.argwhere(got != want)
    assert not len(bad), "%s: %d words differ, first at %s: got %#x, want %#x" % (what, len(bad), tuple(bad[0]), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


def words(X, shape, layout, mods, rng, raw=False, extra=None):
    return ev.edge_block(shape, layout, mods, X.n, rng, X.logn if raw else None, extra)


def last_extra(mods, last):
    """edge lists with the rounding's wrap for the limb that is dropped"""
    return [None] * (len(mods) - 1) + [ev.drop_edges(last)]


# ================================================================ solving inputs with the model
def solve_r(X, c, poly, targets):
    """limb 0 of a canonical polynomial [L][n] changed so that the Montgomery word r of the extension is targets[k % len] at every
    coefficient: the low 32 bits of the conversion sum are linear in limb 0's scaled residue with the odd factor Q / q_0"""
    S, lv = X.S, X.S.lv[c]
    p = [O(x) for x in poly]
    want = np.array([targets[k % len(targets)] for k in range(X.n)], dtype=object)
    rest = 0
    for j in range(1, lv.L):
        rest = rest + p[j] * ksm.MT % lv.q[j] * lv.inv_punct_q[j] % lv.q[j] * lv.punct_q[j]
    y_low = (-want * lv.Q) % ksm.MT                                   # r = -y Q^-1 mod 2^32
    s0 = (y_low - rest) * pow(lv.punct_q[0], -1, ksm.MT) % ksm.MT       # limb 0's scaled residue: these low bits, high bits kept small
    p[0] = s0 * pow(ksm.MT * lv.inv_punct_q[0] % lv.q[0], -1, lv.q[0]) % lv.q[0]
    assert (S.ext_trace(c, p)[1] == want).all()
    return U(p)


def alpha_targets(lv):
    h = lv.m_sk // 2
    return [0] + [v % lv.m_sk for k in range(1, lv.nB + 1) for v in (k, -k)] + [h, h + 1, lv.m_sk - 1, h - 1]


def solve_alpha(X, c, trace, msk_limb, raw):
    """the m_sk limb [n] (written into msk_limb) for which alpha is alpha_targets[k % len] at coefficient k.  trace() -> alpha of the
    current operands; alpha is affine in the m_sk limb's residue with slope -t Q^-1 B^-1"""
    S, lv = X.S, X.S.lv[c]
    tg = alpha_targets(lv)
    want = np.array([tg[k % len(tg)] for k in range(X.n)], dtype=object)
    msk_limb[:] = 0
    a0 = trace() % lv.m_sk
    slope = lv.t * lv.invQ[-1] * lv.invB_msk % lv.m_sk
    d = (a0 - want) * pow(slope, -1, lv.m_sk) % lv.m_sk
    msk_limb[:] = U(S.untwist(d, lv.m_sk, lift=3) if raw else d)
    got = trace() % lv.m_sk
    assert (got == want).all()
    assert {int(v) for v in got} == set(tg)                            # both signs and the boundary itself


def shoup_lazy(x, w, m):
    """x w - floor(x floor(w 2^64 / m) / 2^64) m: the lazy Shoup product (modmath.h), in [0, 2m); m or more only where x w mod m is tiny"""
    return x * w - ((x * ((w << 64) // m)) >> 64) * m


def solve_ext_lazy_sum(X, c, per_limb=4):
    """Canonical coefficients (rows of L residues) for which the unrolled extension's lazy sum v = r' Q/m~ + sum_j xs_j (Q/q_j)/m~ reaches
    4 m on some Bsk limb (behz_ext2_body: v < (2L + 2) m, closed by conditional subtractions of 4 m, 2 m, m).  Four addends below 2 m
    reach 4 m only if every one of them is a lazy product that kept its extra m, i.e. has a tiny residue: the scaled residues xs_j are
    chosen as small multiples of the inverse constants, and the triples are searched for one whose Montgomery word r does the same.
    The search knows the kernel's formulation; the expected values still come from the model."""
    import itertools
    lv = X.S.lv[c]
    assert lv.L == 3 and X.unrolled[c]
    rows = []
    for i, m in enumerate(lv.Bsk):
        w = [pu * lv.inv_mt[i] % m for pu in lv.punct_q]
        wr = lv.Q * lv.inv_mt[i] % m
        cands = []
        for j in range(3):
            xs = [tau * pow(w[j], -1, m) % m for tau in range(1, 24)]
            cands.append([x for x in xs if x < lv.q[j] and shoup_lazy(x, w[j], m) >= m])
        found = 0
        for xs in itertools.product(*cands):
            r = -sum(x * pu for x, pu in zip(xs, lv.punct_q)) * lv.invQ_mt % ksm.MT
            if r < 1 << 31:
                continue
            v = shoup_lazy(r + m - ksm.MT, wr, m) + sum(shoup_lazy(x, wj, m) for x, wj in zip(xs, w))
            if v >= 4 * m:
                rows.append([x * pow(ksm.MT * ip % q, -1, q) % q for x, ip, q in zip(xs, lv.inv_punct_q, lv.q)])
                found += 1
                if found == per_limb:
                    break
    return rows


# ================================================================ the steps
def check_ext(X, c, layout, batch, polys=2):
    lv = X.S.lv[c]
    rng = X.rng(1, c, batch)
    x = words(X, (batch, polys), layout, lv.q, rng)
    if layout == "same":                                              # directed: r on both sides of the centred lift's boundary
        x[0, 0] = solve_r(X, c, x[0, 0], [0, (1 << 31) - 1, 1 << 31, (1 << 32) - 1])
    out = np.zeros((batch, polys, lv.E, X.n), dtype=np.uint64)
    X.run("behz_ext", c, [x], [out], polys=polys, batch=batch)
    same(out, [[X.S.behz_ext(c, list(O(p))) for p in ct] for ct in x], "behz_ext %s L=%d %s" % (X.name, lv.L, layout))


def check_drop_ext(X, c, layout, batch, raw, polys=2):
    S, lv, hi = X.S, X.S.lv[c], X.S.lv[c + 1]
    rng = X.rng(2, c, batch, raw)
    x = words(X, (batch, polys), layout, hi.q, rng, raw, last_extra(hi.q, hi.q[-1]))
    if layout in ("same", "rotated"):
        # directed: the kept residues after the drop are chosen (r at its boundaries), the input is their value times q_last plus a last
        # limb on either side of the rounding's wrap; under RAW as words that stand for these residues
        kept = solve_r(X, c, words(X, (), layout, lv.q, rng), [0, (1 << 31) - 1, 1 << 31, (1 << 32) - 1])
        y = lv.crt(list(O(kept)))
        de = ev.drop_edges(hi.q[-1])
        last = np.array([de[k % len(de)] for k in range(X.n)], dtype=object)
        val = y * hi.q[-1] + ((last + hi.half) % hi.q[-1] - hi.half)  # floor((val + half) / q_last) = y
        limbs = [val % m for m in hi.q]
        assert all((a == b).all() for a, b in zip(S.modswitch(c + 1, limbs), O(kept)))
        x[0, 0] = U([S.untwist(l, m, lift=j + 1) if raw else l for j, (l, m) in enumerate(zip(limbs, hi.q))])
    out = np.zeros((batch, polys, lv.E, X.n), dtype=np.uint64)
    X.run("drop_behz_ext", c, [x], [out], polys=polys, batch=batch, flags=STEP_RAW if raw else 0)
    same(out, [[S.drop_behz_ext(c, list(O(p)), raw) for p in ct] for ct in x], "drop_behz_ext %s L=%d %s raw=%d" % (X.name, lv.L, layout, raw))


def check_tensor(X, c, layout, batch):
    lv = X.S.lv[c]
    rng = X.rng(3, c, batch)
    a, b = words(X, (batch, 2), layout, lv.ext, rng), words(X, (batch, 2), "rotated" if layout == "same" else layout, lv.ext, rng)
    out = np.zeros((batch, 3, lv.E, X.n), dtype=np.uint64)
    X.run("tensor", c, [a, b], [out], batch=batch)
    want = [X.S.tensor(c, [list(O(p)) for p in x], [list(O(p)) for p in y]) for x, y in zip(a, b)]
    same(out, want, "tensor %s L=%d %s" % (X.name, lv.L, layout))
    out2 = np.zeros_like(out)
    X.run("tensor_conv", c, [a, b], [out2], batch=batch, polys=2, terms=2)
    same(out2, want, "tensor_conv %s L=%d %s" % (X.name, lv.L, layout))


def check_tensor_sum(X, c, terms, batch, layout=None):
    """layout None: all four operands of every term at m - 1 on every limb"""
    lv = X.S.lv[c]
    rng = X.rng(4, c, terms)
    if layout is None:
        a = np.ascontiguousarray(np.broadcast_to(np.array([m - 1 for m in lv.ext], dtype=np.uint64)[:, None], (batch, terms, 2, lv.E, X.n)))
        b = a.copy()
    else:
        a, b = words(X, (batch, terms, 2), layout, lv.ext, rng), words(X, (batch, terms, 2), layout, lv.ext, rng)
    want = [X.S.tensor_sum(c, [[list(O(p)) for p in t] for t in x], [[list(O(p)) for p in t] for t in y]) for x, y in zip(a, b)]
    for e0 in (0, lv.L):
        dq = np.full((batch, terms, 3, lv.L, X.n), 7, dtype=np.uint64)
        bs = np.zeros((batch, 3, lv.nB + 1, X.n), dtype=np.uint64)
        X.run("tensor_sum", c, [a, b], [dq if e0 == 0 else None, bs], batch=batch, terms=terms, e0=e0)
        what = "tensor_sum %s L=%d terms=%d e0=%d %s" % (X.name, lv.L, terms, e0, layout)
        same(bs, [w[1] for w in want], what)
        if e0 == 0:
            same(dq, [w[0] for w in want], what)


def finish_operands(X, c, shape, layout, rng, mods):
    """operands of a finish: RAW words on a level with the unrolled kernels, canonical limbs elsewhere"""
    return words(X, shape, layout, mods, rng, raw=X.unrolled[c])


def check_finish(X, c, layout, batch, terms, accumulate):
    S, lv, raw = X.S, X.S.lv[c], X.unrolled[c]
    rng = X.rng(5, c, batch, terms, accumulate)
    d = finish_operands(X, c, (batch, terms, 3), layout, rng, lv.ext)
    if layout in ("same", "rotated"):                                # directed: alpha on every side of its sign split, first term of job 0
        for p in range(3):
            solve_alpha(X, c, lambda: S.finish_trace(c, list(O(d[0, 0, p])), raw)[1], d[0, 0, p, lv.E - 1], raw)
    acc0 = words(X, (batch, 3), "sprinkled", lv.q, rng)
    out = acc0.copy() if accumulate else np.zeros_like(acc0)
    X.run("behz_finish", c, [d], [out], batch=batch, terms=terms, flags=(STEP_RAW if raw else 0) | (STEP_ACCUMULATE if accumulate else 0))
    want = [[S.behz_finish(c, [list(O(d[b, t, p])) for t in range(terms)], raw, list(O(acc0[b, p])) if accumulate else None) for p in range(3)]
            for b in range(batch)]
    same(out, want, "behz_finish %s L=%d nB=%d %s terms=%d acc=%d" % (X.name, lv.L, lv.nB, layout, terms, accumulate))


def finish_sum_bound(lv):
    """terms * q_widest < 2^63 (eval_plan.h, p.summed)"""
    return ((1 << 63) - 1) // max(lv.q)


def check_finish_sum(X, c, layout, batch, terms, at_bound=False):
    S, lv, raw = X.S, X.S.lv[c], X.unrolled[c]
    rng = X.rng(6, c, batch, terms)
    dq = finish_operands(X, c, (batch, terms, 3), layout, rng, lv.q)
    bs = finish_operands(X, c, (batch, 3), layout, rng, lv.Bsk)
    if at_bound:                                                      # every per-term scaled canonical residue is q_j - 1
        for j, m in enumerate(lv.q):
            v = (m - 1) * pow(lv.t * lv.inv_punct_q[j] % m, -1, m) % m
            col = np.full(X.n, v, dtype=object)
            dq[:, :, :, j, :] = U(S.untwist(col, m, lift=2) if raw else col)
        assert all((x == m - 1).all() for x, m in zip(S.scaled_q(c, S.canon(list(O(dq[0, 0, 0])), lv.q, raw)), lv.q))
    if layout in ("same", "rotated") or at_bound:
        for p in range(3):
            solve_alpha(X, c, lambda: S.finish_sum_trace(c, [list(O(dq[0, t, p])) for t in range(terms)], list(O(bs[0, p])), raw)[1], bs[0, p, lv.nB], raw)
    out = np.zeros((batch, 3, lv.L, X.n), dtype=np.uint64)
    X.run("behz_finish_sum", c, [dq, bs], [out], batch=batch, terms=terms, flags=STEP_RAW if raw else 0)
    want = [[S.behz_finish_sum(c, [list(O(dq[b, t, p])) for t in range(terms)], list(O(bs[b, p])), raw) for p in range(3)] for b in range(batch)]
    same(out, want, "behz_finish_sum %s L=%d nB=%d %s terms=%d" % (X.name, lv.L, lv.nB, layout, terms))


def check_ks(X, c, layout, batch, all_max=False):
    """ks_inner, then ks_moddown (plain and RAW, with and without the fused extension) on edge words of its own"""
    S, lv, K = X.S, X.S.lv[c], X.S.K
    L, mods = lv.L, X.S.acc_mods(c)
    rng = X.rng(7, c, batch)
    td_mods = [m for m in mods for _ in range(L)]
    if all_max:
        tdec = np.ascontiguousarray(np.broadcast_to(np.array([m - 1 for m in td_mods], dtype=np.uint64).reshape(L + 1, L)[:, :, None], (batch, L + 1, L, X.n)))
        rk = np.ascontiguousarray(np.broadcast_to(np.array([m - 1 for m in X.S.key_q], dtype=np.uint64)[None, None, :, None], (K - 1, 2, K, X.n)))
    else:
        tdec = words(X, (batch,), layout, td_mods, rng).reshape(batch, L + 1, L, X.n)
        rk = words(X, (K - 1, 2), layout, X.S.key_q, rng)
    acc = np.zeros((batch, 2, L + 1, X.n), dtype=np.uint64)
    X.run("ks_inner", c, [tdec, rk], [acc], batch=batch)
    same(acc, [S.ks_inner(c, O(t), O(rk)) for t in tdec], "ks_inner %s L=%d %s max=%d" % (X.name, L, layout, all_max))
    if all_max:
        return
    for raw in (False, True):
        if raw and L > 4:
            continue                                                  # refused: test_refusals
        a = words(X, (batch, 2), layout, mods, rng, raw, last_extra(mods, mods[-1]))
        if raw and layout in ("same", "rotated"):                     # words that stand for the residues at the rounding's wrap
            can = words(X, (2,), layout, mods, rng, False, last_extra(mods, mods[-1]))
            a[0] = U([[S.untwist(O(l), m, lift=j) for j, (l, m) in enumerate(zip(p, mods))] for p in can])
        for polys, n_ext in ((2, 0), (3, 0)) + (((2, min(batch, 2)),) if X.unrolled[c] else ()):
            ct0 = words(X, (batch, polys), "sprinkled", lv.q, rng)
            if n_ext and layout in ("same", "rotated"):
                # the fused extension sees ct + round(acc / p): with acc standing for zero the result is ct, whose r word is solved
                a[0] = 0
                ct0[0, 0] = solve_r(X, c, ct0[0, 0], [0, (1 << 31) - 1, 1 << 31, (1 << 32) - 1])
            ct = ct0.copy()
            ext = np.zeros((n_ext, 2, lv.E, X.n), dtype=np.uint64) if n_ext else None
            X.run("ks_moddown", c, [a], [ct, ext], batch=batch, polys=polys, n_ext=n_ext, flags=STEP_RAW if raw else 0)
            want = [S.ks_moddown(c, [list(O(p)) for p in a[b]], [list(O(p)) for p in ct0[b, :2]], raw) for b in range(batch)]
            what = "ks_moddown %s L=%d %s raw=%d polys=%d n_ext=%d" % (X.name, L, layout, raw, polys, n_ext)
            same(ct[:, :2], want, what)
            assert (ct[:, 2:] == ct0[:, 2:]).all(), what
            if n_ext:
                same(ext, [[S.behz_ext(c, p) for p in w] for w in want[:n_ext]], what + " ext")


def check_modswitch(X, c, layout, batch, polys=2):
    lv = X.S.lv[c]
    rng = X.rng(8, c, batch)
    x = words(X, (batch, polys), layout, lv.q, rng, False, last_extra(lv.q, lv.q[-1]))
    want = [[X.S.modswitch(c, list(O(p))) for p in ct] for ct in x]
    for step in ("modswitch", "modswitch_jobs"):
        out = np.zeros((batch, polys, lv.L - 1, X.n), dtype=np.uint64)
        X.run(step, c, [x], [out], batch=batch, polys=polys)
        same(out, want, "%s %s L=%d %s" % (step, X.name, lv.L, layout))


def i0_bound(lv):
    """the largest terms with (terms + 1) * q_last < 2^64 (eval_plan.h, p.i0_fast)"""
    return (W64 - 1) // lv.q[-1] - 1


def check_i0(X, c, layout, batch, terms, raw, store, at_bound=False):
    S, lv = X.S, X.S.lv[c]
    kept, ql = lv.q[:-1], lv.q[-1]
    rng = X.rng(9, c, batch, terms, raw, store)
    s = words(X, (batch, 2), layout, kept, rng, raw)
    v = words(X, (batch, terms, 2), layout, [ql], rng, raw, [ev.drop_edges(ql)])
    if at_bound:                                                      # every (v + half) mod q_last is q_last - 1
        col = np.full(X.n, ql - 1 - lv.half, dtype=object)
        v[:] = U(S.untwist(col, ql, lift=1) if raw else col)
    elif raw and layout in ("same", "rotated"):
        can = words(X, (terms, 2), layout, [ql], rng, False, [ev.drop_edges(ql)])
        v[0] = U([[[S.untwist(O(l), ql, lift=2) for l in p] for p in t] for t in can])
    acc0 = words(X, (batch, 2), "sprinkled", kept, rng)
    out = acc0.copy()
    X.run("i0_finish", c, [s, v], [out], batch=batch, terms=terms, flags=(STEP_RAW if raw else 0) | (STEP_STORE if store else 0))
    want = [[S.i0_finish(c, list(O(s[b, p])), [O(v[b, t, p, 0]) for t in range(terms)], list(O(acc0[b, p])), raw, store) for p in range(2)] for b in range(batch)]
    same(out, want, "i0_finish %s L=%d %s terms=%d raw=%d store=%d" % (X.name, lv.L, layout, terms, raw, store))


def plain_edges(X, rng, batch):
    """plaintext coefficients: 0, 1, t - 1, (t +- 1) / 2 per coefficient, then random"""
    t = X.t
    kinds = np.array([0, 1, t - 1, (t - 1) // 2, (t + 1) // 2, t - 2, (t + 3) // 2], dtype=np.uint64)
    out = rng.integers(0, t, (batch, X.n), dtype=np.uint64)
    out[0] = kinds[np.arange(X.n) % len(kinds)]
    if batch > 1:
        out[1] = kinds[(np.arange(X.n) // len(kinds)) % len(kinds)]
    return out


def check_plain(X, c, layout, batch):
    """add_plain, lift, dyadic_plain, add_many, sum_jobs"""
    S, lv = X.S, X.S.lv[c]
    rng = X.rng(10, c, batch)
    pt = plain_edges(X, rng, batch)
    c0 = words(X, (batch,), layout, lv.q, rng)
    out = c0.copy()
    X.run("add_plain", c, [pt], [out], batch=batch)
    same(out, [S.add_plain(c, list(O(x)), O(m)) for x, m in zip(c0, pt)], "add_plain %s L=%d %s" % (X.name, lv.L, layout))
    flags = np.array([b % 2 for b in range(batch)], dtype=np.uint64)
    for nl in (None, flags):
        out = np.zeros((batch, lv.L, X.n), dtype=np.uint64)
        X.run("lift", c, [pt, nl], [out], batch=batch)
        same(out, [S.lift(c, O(m), nl is not None and bool(nl[b])) for b, m in enumerate(pt)], "lift %s L=%d" % (X.name, lv.L))
    ct, p2 = words(X, (batch, 2), layout, lv.q, rng), words(X, (batch,), "rotated", lv.q, rng)
    out = np.zeros_like(ct)
    X.run("dyadic_plain", c, [ct, p2], [out], batch=batch, polys=2)
    same(out, [[[x * y % m for x, y, m in zip(O(p), O(pl), lv.q)] for p in cb] for cb, pl in zip(ct, p2)], "dyadic_plain %s L=%d %s" % (X.name, lv.L, layout))
    terms = 5
    x = words(X, (batch, terms, 2), layout, lv.q, rng)
    sums = [[[sum(O(x[b, :, p, j])) % m for j, m in enumerate(lv.q)] for p in range(2)] for b in range(batch)]
    acc0 = words(X, (batch, 2), "max_one", lv.q, rng)
    out = acc0.copy()
    X.run("add_many", c, [x], [out], batch=batch, terms=terms, polys=2)
    same(out, [[[(a + s) % m for a, s, m in zip(O(ap), sp, lv.q)] for ap, sp in zip(acc0[b], sums[b])] for b in range(batch)], "add_many %s L=%d %s" % (X.name, lv.L, layout))
    out = np.zeros_like(acc0)
    X.run("sum_jobs", c, [x], [out], batch=batch, terms=terms, polys=2)
    same(out, sums, "sum_jobs %s L=%d %s" % (X.name, lv.L, layout))


def check_epilogue(X, c, layout, batch, adds, key):
    S, lv = X.S, X.S.lv[c]
    rng = X.rng(11, c, batch, adds, key)
    ct = words(X, (batch, 2), layout, lv.q, rng, False, last_extra(lv.q, lv.q[-1]))
    a0, mask = plain_edges(X, rng, batch), plain_edges(X, rng, batch)[::-1].copy()
    add = [np.ascontiguousarray(np.broadcast_to(np.array([m - 1 for m in lv.q], dtype=np.uint64)[:, None], (batch, 2, lv.L, X.n))) if i < adds else None for i in range(2)]
    ks, ct_in = None, ct
    if key:
        mods = S.acc_mods(c)
        ks = words(X, (batch, 2), layout, mods, rng, True, last_extra(mods, mods[-1]))
        # the fused form equals ks_moddown (raw) followed by the epilogue without a key
        ct_in = U([S.ks_moddown(c, [list(O(p)) for p in ks[b]], [list(O(p)) for p in ct[b]], raw=True) for b in range(batch)]).reshape(ct.shape)
    out = np.zeros((batch, 2, X.n), dtype=np.uint64)
    X.run("eval_epilogue", c, [ct, a0, mask, add[0], add[1], ks], [out], batch=batch, flags=STEP_KEY if key else 0)
    want = [S.eval_epilogue(c, [list(O(p)) for p in ct_in[b]], O(a0[b]), O(mask[b]), None if add[0] is None else [list(O(p)) for p in add[0][b]],
                            None if add[1] is None else [list(O(p)) for p in add[1][b]], X.clear_bits) for b in range(batch)]
    what = "eval_epilogue %s L=%d %s adds=%d key=%d" % (X.name, lv.L, layout, adds, key)
    same(out, want, what)
    if key:
        md = ct.copy()
        X.run("ks_moddown", c, [ks], [md, None], batch=batch, polys=2, flags=STEP_RAW)
        out2 = np.zeros_like(out)
        X.run("eval_epilogue", c, [md, a0, mask, add[0], add[1], None], [out2], batch=batch)
        assert (out2 == out).all(), what + ": fused and unfused differ"


# ================================================================ tests
@pytest.mark.parametrize("layout", ev.LAYOUTS)
@pytest.mark.parametrize("name", ALL_CHAINS + ["60x5"])
def test_behz_ext_and_drop_ext(ctx, name, layout):
    """k_behz_ext2<1..3, DROP, RAW>, k_behz_ext<4,4>, k_behz_ext<0,0>: every level of the chain"""
    X = ctx(name)
    for c in levels_of(name):
        check_ext(X, c, layout, 3)
        if X.unrolled[c] and c + 1 <= X.first:
            for raw in (False, True):
                check_drop_ext(X, c, layout, 3, raw)


@pytest.mark.parametrize("name", ["60x5", "60x5-seal-aux"])
def test_behz_ext_lazy_sum_reaches_four_m(ctx, name):
    """L = 3: coefficients whose lazy sum is 4 m or more, so the first of the three closing subtractions is taken (solve_ext_lazy_sum);
    through launch_behz_ext, the fused drop and the mod-down's fused extension"""
    X = ctx(name)
    c, S = 2, X.S
    lv, hi = S.lv[c], S.lv[c + 1]
    rows = solve_ext_lazy_sum(X, c)
    assert len(rows) >= 2, "no coefficient reaches 4 m on %s" % name
    x = words(X, (1, 1), "sprinkled", lv.q, X.rng(12))
    for k, row in enumerate(rows):
        x[0, 0, :, k] = row
    out = np.zeros((1, 1, lv.E, X.n), dtype=np.uint64)
    X.run("behz_ext", c, [x], [out], polys=1, batch=1)
    want = [[S.behz_ext(c, list(O(x[0, 0])))]]
    same(out, want, "behz_ext at 4 m, " + name)
    # the same residues behind a drop (their value times q_last, last limb 0) and behind a mod-down of sums that stand for zero
    val = lv.crt(list(O(x[0, 0]))) * hi.q[-1]
    for raw in (False, True):
        xin = U([[[S.untwist(val % m, m, lift=1) if raw else val % m for m in hi.q]]])
        out = np.zeros((1, 1, lv.E, X.n), dtype=np.uint64)
        X.run("drop_behz_ext", c, [xin], [out], polys=1, batch=1, flags=STEP_RAW if raw else 0)
        same(out, want, "drop_behz_ext at 4 m, %s raw=%d" % (name, raw))
        ct = np.ascontiguousarray(np.stack([x[0, 0], x[0, 0]])[None])
        ext = np.zeros((1, 2, lv.E, X.n), dtype=np.uint64)
        X.run("ks_moddown", c, [np.zeros((1, 2, lv.L + 1, X.n), dtype=np.uint64)], [ct, ext], polys=2, batch=1, n_ext=1, flags=STEP_RAW if raw else 0)
        same(ext, [[want[0][0], want[0][0]]], "ks_moddown's extension at 4 m, %s raw=%d" % (name, raw))


@pytest.mark.parametrize("layout", ev.LAYOUTS)
@pytest.mark.parametrize("name", ALL_CHAINS)
def test_tensor_and_tensor_conv(ctx, name, layout):
    X = ctx(name)
    check_tensor(X, X.first, layout, 3)
    check_tensor(X, 0, layout, 1)


@pytest.mark.parametrize("terms", [1, 7, 8, 9, 16, 17])
@pytest.mark.parametrize("name", ["60x4", "60x4-seal-aux", "50x6", "60x3-t41"])
def test_tensor_sum_all_operands_at_their_maximum(ctx, name, terms):
    """the 128-bit sums are folded every 8 terms: all four operands of every term at m - 1 on every limb, e0 = 0 and e0 = L"""
    X = ctx(name)
    check_tensor_sum(X, X.first, terms, 1)


@pytest.mark.parametrize("layout", ev.LAYOUTS)
@pytest.mark.parametrize("name", ["60x4", "60x4-seal-aux", "48x8"])
def test_tensor_sum_layouts(ctx, name, layout):
    X = ctx(name)
    check_tensor_sum(X, X.first, 9, 3, layout)


def test_tensor_sum_61_bit_limbs_far_past_the_fold(ctx):
    """SEAL's 61-bit auxiliary base, 64 and 65 terms at m - 1: 128 products of nearly 2^122 pass through each sum between folds of 8"""
    X = ctx("60x4-seal-aux")
    assert all(m.bit_length() == 61 for m in X.S.lv[X.first].Bsk)
    for terms in (64, 65):
        check_tensor_sum(X, X.first, terms, 1)


@pytest.mark.parametrize("layout", ev.LAYOUTS)
@pytest.mark.parametrize("name", ALL_CHAINS)
def test_behz_finish(ctx, name, layout):
    """k_behz_finish2<1..3> (RAW), k_behz_finish<4,4>, k_behz_finish<0,0>: store and accumulate, one and three terms"""
    X = ctx(name)
    for c in levels_of(name):
        if c > 3 and c != X.first:
            continue                                                  # generic levels: the first one has them all
        check_finish(X, c, layout, 3, 1, False)
        check_finish(X, c, layout, 1, 3, True)


@pytest.mark.parametrize("layout", ev.LAYOUTS)
@pytest.mark.parametrize("name", ALL_CHAINS)
def test_behz_finish_sum(ctx, name, layout):
    """k_behz_finish_sum<1..3, true> (RAW), <4, false>, <0, false>"""
    X = ctx(name)
    for c in levels_of(name):
        if c > 3 and c != X.first:
            continue
        check_finish_sum(X, c, layout, 3, 2)


@pytest.mark.parametrize("name", ALL_CHAINS)
def test_behz_finish_sum_at_the_term_bound(ctx, name):
    """terms at the host-checked bound of the chain's widest prime (64 where the bound is larger: data size), every per-term scaled
    residue q_j - 1; one term more is refused"""
    X = ctx(name)
    for c in sorted({X.first, min(X.first, 2), 0}):
        lv = X.S.lv[c]
        bound = finish_sum_bound(lv)
        check_finish_sum(X, c, "sprinkled", 1, min(bound, 64), at_bound=True)
        assert bound + 1 < 1 << 31
        tok = np.zeros(X.n, dtype=np.uint64)                          # the bound is checked before the sizes
        with pytest.raises(ValueError, match="2\\^63"):
            X.run("behz_finish_sum", c, [tok, tok], [tok], terms=bound + 1, flags=STEP_RAW if X.unrolled[c] else 0)


@pytest.mark.parametrize("layout", ev.LAYOUTS)
@pytest.mark.parametrize("name", ALL_CHAINS)
def test_key_switch_steps(ctx, name, layout):
    """k_ks_inner<1..4>, <0>; k_ks_moddown<TL, EXT, RAW> in every combination the launcher has"""
    X = ctx(name)
    for c in levels_of(name):
        if c > 4 and c != X.first:
            continue
        check_ks(X, c, layout, 3)


@pytest.mark.parametrize("name,c", [("60x4", 0), ("50x6", 3), ("50x6", 4), ("48x8", 6)])
def test_ks_inner_every_word_at_its_maximum(ctx, name, c):
    """L = 1, 4, 5, 7: every decomposed limb and every key word m - 1"""
    check_ks(ctx(name), c, "same", 1, all_max=True)


@pytest.mark.parametrize("layout", ev.LAYOUTS)
@pytest.mark.parametrize("name", ALL_CHAINS)
def test_modswitch(ctx, name, layout):
    """barrett64(last, m) with the dropped prime narrower and wider than the kept ones (the mixed chains)"""
    X = ctx(name)
    for c in range(1, X.first + 1):
        check_modswitch(X, c, layout, 3)


@pytest.mark.parametrize("layout", ev.LAYOUTS)
@pytest.mark.parametrize("name", ALL_CHAINS)
def test_i0_finish(ctx, name, layout):
    X = ctx(name)
    for c in sorted({X.first, 1}):
        for raw in (False, True):
            for store in (False, True):
                check_i0(X, c, layout, 3, 4, raw, store)


@pytest.mark.parametrize("name", ALL_CHAINS)
def test_i0_finish_at_the_term_bound(ctx, name):
    """the largest terms with (terms + 1) * q_last < 2^64 (64 where that is larger), every (v + half) mod q_last = q_last - 1; one more is refused"""
    X = ctx(name)
    c = X.first
    lv = X.S.lv[c]
    bound = i0_bound(lv)
    for raw in (False, True):
        for store in (False, True):
            check_i0(X, c, "sprinkled", 1, min(bound, 64), raw, store, at_bound=True)
    if bound + 1 < 1 << 31:                                           # (a 30-bit last prime: one past the bound is no 32-bit term count)
        tok = np.zeros(X.n, dtype=np.uint64)                          # the bound is checked before the sizes
        with pytest.raises(ValueError, match="2\\^64"):
            X.run("i0_finish", c, [tok, tok], [tok], terms=bound + 1)


@pytest.mark.parametrize("layout", ev.LAYOUTS)
@pytest.mark.parametrize("name", ALL_CHAINS)
def test_plain_and_sum_steps(ctx, name, layout):
    """add_plain and lift (the 41-bit plain modulus takes the shift-subtract division), dyadic_plain, add_many, sum_jobs"""
    X = ctx(name)
    for c in sorted({X.first, 0}):
        check_plain(X, c, layout, 3)


@pytest.mark.parametrize("layout", ev.LAYOUTS)
@pytest.mark.parametrize("name", ALL_CHAINS)
def test_eval_epilogue(ctx, name, layout):
    """with and without addends at q - 1, with and without the fused key-switch mod-down, from levels that drop one and several limbs"""
    X = ctx(name)
    for c in sorted({min(X.first, 3), 1, 0}):
        check_epilogue(X, c, layout, 3, 0, False)
        check_epilogue(X, c, layout, 1, 2, True)
    check_epilogue(X, X.first, layout, 1, 1, False)


@pytest.mark.parametrize("name", ALL_CHAINS + ["60x4-seal-aux"])
def test_every_step_below_one_workgroup(ctx, name):
    """n = 64 < EW_T: the tail guard of every kernel, one job"""
    X = ctx(name, 64)
    c = X.first
    check_ext(X, c, "same", 1)
    if X.unrolled[c - 1]:
        for raw in (False, True):
            check_drop_ext(X, c - 1, "rotated", 1, raw)
    check_tensor(X, c, "rotated", 1)
    check_tensor_sum(X, c, 9, 1, "sprinkled")
    check_finish(X, c, "same", 1, 2, True)
    check_finish_sum(X, c, "rotated", 1, 2)
    check_ks(X, c, "same", 1)
    check_modswitch(X, c, "rotated", 1)
    check_i0(X, c, "same", 1, 3, c + 1 <= 4, False)
    check_plain(X, c, "same", 1)
    check_epilogue(X, c, "rotated", 1, 1, c + 1 <= 4)


def test_refusals(ctx):
    """what a launcher cannot take is refused with a reason, never launched"""
    X, Y, Z = ctx("60x4"), ctx("50x6"), ctx("60x3-t41")
    n = X.n
    z = lambda *shape: np.zeros(shape + (n,), dtype=np.uint64)
    with pytest.raises(ValueError, match="not a data level"):
        X.run("behz_ext", 3, [z(1, 2, 4)], [z(1, 2, 9)], polys=2)
    with pytest.raises(ValueError, match="wrong size"):
        X.run("behz_ext", 2, [z(1, 2, 2)], [z(1, 2, 7)], polys=2)
    with pytest.raises(ValueError, match="not a canonical residue"):
        X.run("behz_ext", 2, [np.full((1, 2, 3, n), W64 - 1, dtype=np.uint64)], [z(1, 2, 7)], polys=2)
    with pytest.raises(ValueError, match="unrolled sizes only"):                     # launch_drop_behz_ext where behz_unrolled is false
        Y.run("drop_behz_ext", 3, [z(1, 2, 5)], [z(1, 2, 9)], polys=2, flags=STEP_RAW)
    with pytest.raises(ValueError, match="unrolled sizes only"):
        Z.run("drop_behz_ext", 0, [z(1, 2, 2)], [z(1, 2, 4)], polys=2)
    with pytest.raises(ValueError, match="no RAW form above four limbs"):            # launch_ks_moddown raw with L > 4
        Y.run("ks_moddown", 4, [z(1, 2, 6)], [z(1, 2, 5), None], polys=2, flags=STEP_RAW)
    with pytest.raises(ValueError, match="fused extension"):
        Y.run("ks_moddown", 3, [z(1, 2, 5)], [z(1, 2, 4), z(1, 2, 9)], polys=2, n_ext=1)
    with pytest.raises(ValueError, match="RAW input only"):
        X.run("behz_finish", 2, [z(1, 1, 3, 7)], [z(1, 3, 3)], terms=1)
    with pytest.raises(ValueError, match="no RAW form"):
        Y.run("behz_finish", 4, [z(1, 1, 3, 11)], [z(1, 3, 5)], terms=1, flags=STEP_RAW)
    with pytest.raises(ValueError, match="RAW key-switch|at most four limbs"):
        Y.run("eval_epilogue", 4, [z(1, 2, 5), z(1), z(1), None, None, z(1, 2, 6)], [z(1, 2)], flags=STEP_KEY)
    with pytest.raises(ValueError, match="end of the modulus switching chain"):
        X.run("modswitch", 0, [z(1, 2, 1)], [z(1, 2, 0)], polys=2)
    with pytest.raises(ValueError, match="unknown step"):
        a = E._StepArgs()
        a.step, a.batch = 99, 1
        E._check(E.load_library().apsu_he_debug_run_step(X.G.h, C.byref(a)))
