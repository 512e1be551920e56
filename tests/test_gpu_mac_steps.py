"""GPU tier: every multiply-accumulate and packed-row kernel alone, one launch at a time, bit for bit against tests/mac_step_model.py.

apsu_he_debug_run_step's MAC_INFO / MAC / TERM_PRODUCT / PACK_ROWS / UNPACK_ROWS / LIMB0_ROWS steps (include/apsu_he.h) put chosen
words in front of ONE launch_mac, launch_term_product, launch_pack_rows, launch_unpack_rows or launch_limb0_rows with the context's
own level block.  The cases are mac_step_model's -- the same generator tests/test_mac_step_model_cpu.py feeds to the CPU emulation of
the kernels' lanes -- so what runs here is the gfx950 build of a text that is known to agree with the model when compiled for the
host: v_alignbit, the kept sums' register constraints, the 4-byte-aligned 16-byte loads, the grid decode on real block indices.
Every comparison is exact; nothing is skipped.

What the public API's route (n = 8192, the shapes an evaluation produces) never runs, and the test that does:
  limb_slow = 0 (mac_grid picks it above 65 535 jobs only)            test_mac_worst_case_chains, test_mac_directed (both orders, a handful of jobs)
  limb0 != 0                                                          test_mac_directed, test_term_product_every_limb (the chain of one term)
  nl below L with three different strides, P above L                  test_mac_directed
  limbs of different row widths (unequal mac_row_off / mac_chunk)     test_mac_info, test_mac_worst_case_chains[mixed], test_mac_directed[mixed], test_rows[mixed]
  row widths other than 32 and 48 .. (33, 36, 51 -> 52, 55 -> 56)     test_mac_info, test_mac_worst_case_chains[36x3 / mixed], test_rows
  k_term_product alone, its second z slab, the u >= njobs guard       test_term_product_every_limb, test_term_product_second_z_slab
  k_pack_rows / k_unpack_rows / k_limb0_rows alone                    test_rows
  all of it below one workgroup (k >= n)                              the n = 64 pass of each

Shapes: n = 1024 is two blocks of 256 lanes, and at 49 bits one block already meets every even shift of the 16-byte window
(test_window_shifts_at_49_bits below keeps the claim); n = 64 is a quarter of a block, the tail guard.  58- and 60-bit primes are
stored in 64-bit rows: a context of them alone has no packed form (refused, test_refusals), so those chains run dense, and the 64-bit
row next to packed ones is "36-36-60".  The context admits every prime the chains ask for; no width had to be replaced."""
import numpy as np
import pytest

import apsu_amd
import edge_values as ev
import mac_step_model as M
from apsu_amd.engine import STEP_KARA, STEP_LIMB_SLOW, STEP_PACKED

pytestmark = pytest.mark.gpu

ALL_CHAINS = list(M.CHAINS)
INFO = ("mac_shift", "mac_chunk", "mac_chunk_k", "mac_bits", "mac_row_off", "mac_mask_hi", "kara_usable")


class Ctx:
    def __init__(self, name, n):
        q, t, L = M.chain(name, n)
        self.name, self.n, self.L, self.c, self.qs = name, n, L, L - 1, q[:L]
        self.G = apsu_amd.HeContext(n=n, coeff_modulus=q, plain_modulus=t)
        self.rows = M.Rows(self.qs, n)
        self.any_packed = any(w != 64 for w in self.rows.bits)
        self.kara = all(ev.mac_chunk_kara(v) for v in self.qs)

    def step(self, step, ins, out, **kw):
        self.G.debug_run_step(step, self.c, ins=ins, outs=[out], **kw)
        return out

    def forms(self):
        """(three-product, packed, limb_slow) this level can be launched in"""
        return [(k, p, s) for k in ((0, 1) if self.kara else (0,)) for p in ((0, 1) if self.any_packed else (0,)) for s in (0, 1)]

    def slots(self, dense, packed):
        """plaintext slots [..][L][n] as the step takes them"""
        return self.rows.words(dense.reshape(-1, self.L, self.n)) if packed else np.ascontiguousarray(dense)

    def mac(self, case, kara, packed, limb_slow, pt=None):
        flags = (STEP_KARA if kara else 0) | (STEP_PACKED if packed else 0) | (STEP_LIMB_SLOW if limb_slow else 0)
        pt = self.slots(case.coeffs, packed) if pt is None else pt
        return self.step("mac", [case.powers, pt, case.job_table()], case.out0(), flags=flags, terms=case.terms, polys=case.polys, batch=case.batch,
                         e0=0 if case.table else case.jobs[0][0], n_ext=case.NL)

    def mac_all_forms(self, case):
        pts = {p: self.slots(case.coeffs, p) for p in {f[1] for f in self.forms()}}          # packed once per case
        for kara, packed, limb_slow in self.forms():
            out = self.mac(case, kara, packed, limb_slow, pts[packed])
            assert case.wrong(out) == [], "%s n %d %s: three-product %d packed %d limb_slow %d (job, stream, polynomial, limb)" % (
                self.name, self.n, case.name, kara, packed, limb_slow)


_CTX = {}


@pytest.fixture(scope="module")
def ctx():
    def get(name, n=1024):
        if (name, n) not in _CTX:
            _CTX[(name, n)] = Ctx(name, n)
        return _CTX[(name, n)]
    yield get
    for X in _CTX.values():
        X.G.close()
    _CTX.clear()


# ================================================================ mac_info: the level block the kernels read
@pytest.mark.parametrize("name", ALL_CHAINS)
@pytest.mark.parametrize("n", [1024, 64])
def test_mac_info(ctx, name, n):
    """first: the intended widths are what is stored, and every constant of the device's block is the model's"""
    X = ctx(name, n)
    out = X.step("mac_info", [], np.zeros(2 + 7 * X.L, dtype=np.uint64))
    v = [int(x) for x in out]
    info = {k: v[2 + i::7] for i, k in enumerate(INFO)}
    assert v[0] == X.L and v[1] == X.rows.slot_bytes == n * sum(info["mac_bits"]) // 8 and v[1] % 8 == 0
    assert info["mac_bits"] == M.STORED[name] == [M.row_bits(q) for q in X.qs]
    assert info["mac_shift"] == [ev.mac_shift(q) for q in X.qs] and info["mac_chunk"] == [ev.mac_chunk(q) for q in X.qs]
    for j, q in enumerate(X.qs):
        usable = ev.mac_chunk_kara(q) != 0
        assert info["kara_usable"][j] == int(usable)
        if usable:
            assert info["mac_chunk_k"][j] == ev.mac_chunk_kara(q)
        w, s = info["mac_bits"][j], info["mac_shift"][j]
        assert info["mac_row_off"][j] == sum(n * b // 8 for b in info["mac_bits"][:j])       # the running sum
        assert info["mac_mask_hi"][j] == ((1 << 32) - 1 if w == 64 else (1 << (w - s)) - 1)
        assert M.windows_fit(w, n)
    if name == "mixed" and n == 64:
        assert [o % 16 for o in info["mac_row_off"][1:3]] == [8, 8]                           # rows that start off the 16-byte grid


def test_window_shifts_at_49_bits():
    """256 lanes of a 49-bit row meet every even shift of the 16-byte window: one block of the n = 1024 cases does"""
    assert {(k // 2) * 2 * 49 % 32 for k in range(0, 512, 2)} == set(range(0, 32, 2))


# ================================================================ k_mac
@pytest.mark.parametrize("name", M.EQUAL_CHAINS + ["36-36-60", "mixed"])
def test_mac_worst_case_chains(ctx, name):
    """chains around each chunk (chain_lengths; one chain of 200 terms where the chunk is thousands) and of 1, 2 and 3 terms, 1, 3 and
    4 streams with different data, fills of edge_values on both operands; both forms where usable, dense and packed, both grid orders"""
    X = ctx(name, 1024)
    for case in M.worst_case_launches(X.qs, 1024, seed=len(name) + 1024):
        X.mac_all_forms(case)


@pytest.mark.parametrize("name", M.EQUAL_CHAINS + ["36-36-60", "mixed"])
def test_mac_worst_case_chains_below_one_workgroup(ctx, name):
    """n = 64: 32 lanes work, 224 leave at k >= n; the same chain lengths"""
    X = ctx(name, 64)
    for case in M.worst_case_launches(X.qs, 64, seed=len(name) + 64):
        X.mac_all_forms(case)


@pytest.mark.parametrize("name", M.DIRECTED_CHAINS)
@pytest.mark.parametrize("n", [1024, 64])
def test_mac_directed(ctx, name, n):
    """(limb0, nl) = (0, L), (0, L - 1), (1, L - 1), (L - 1, 1) with P = L and L + 3: the output is indexed by the limb's position in the
    window, the operands by the limb, and out_poly_stride = nl n, pw_poly_stride = P n and the slot's stride all differ.  Then a table
    of six jobs whose windows, stream counts and chain lengths differ, over pattern-filled outputs: the limbs a job does not handle
    (workgroups that leave at b_limb >= nl), the streams it does not have and every other job's output come back untouched"""
    X = ctx(name, n)
    cases = M.directed_launches(X.qs, n, seed=n)
    assert {(c.jobs[0][0], c.jobs[0][1], c.P) for c in cases if not c.table} == {(a, b, P) for a, b in M.limb_windows(X.L) for P in (X.L, X.L + 3)}
    tables = [c for c in cases if c.table]
    assert len(tables) == 2 and all(len(c.jobs) >= 5 and len({j[:2] for j in c.jobs}) >= 5 for c in tables)
    for case in cases:
        assert (case.expected() == M.PATTERN).any() == case.table
        X.mac_all_forms(case)


# ================================================================ k_term_product
def run_term(X, T, packed):
    return X.step("term_product", [T.powers, X.slots(T.coeffs, packed)], T.out0(), flags=STEP_PACKED if packed else 0, terms=T.repeat, batch=T.batch, e0=T.limb)


@pytest.mark.parametrize("name", ["mixed", "50x3", "56x4", "60x3"])
@pytest.mark.parametrize("n", [1024, 64])
def test_term_product_every_limb(ctx, name, n):
    """dense and packed on every limb: equals the model, equals the MAC step with one term on the same operands (limb0 = the limb,
    nl = 1), and the guard behind the last job's output keeps its pattern"""
    X = ctx(name, n)
    for limb in range(X.L):
        T = M.TermCase(X.qs, n, limb, batch=3, repeat=2, seed=[n, limb], P=X.L + (limb % 2) * 3)
        chain_case = T.as_mac_case()
        for packed in ((0, 1) if X.any_packed else (0,)):
            out = run_term(X, T, packed)
            assert (out == T.expected()).all() and (out[-1] == M.PATTERN).all(), (name, n, limb, packed)
            mac = X.mac(chain_case, 0, packed, 1).reshape(T.batch, 2, n)
            assert (mac == out[:T.batch]).all(), (name, n, limb, packed)


@pytest.mark.parametrize("packed", [0, 1])
def test_term_product_second_z_slab(ctx, packed):
    """n = 64, 32 775 jobs (32 768 + 5 and two more: three operand sets, each repeated 10 925 times): the grid's y is 32 768, seven jobs lie
    in the second z slab and the rest of that slab leaves at u >= njobs.  Every job's [2][n] is checked (34 MB), and the guard
    behind the last one -- where a lane that took entry njobs of the table for a job would most likely store -- keeps its pattern"""
    X = ctx("mixed", 64)
    T = M.TermCase(X.qs, 64, 1, batch=3, repeat=(32768 + 5) // 3 + 1, seed=7)
    assert T.njobs == 32775
    out = run_term(X, T, packed)
    assert (out == T.expected()).all() and (out[-1] == M.PATTERN).all()


# ================================================================ k_pack_rows, k_unpack_rows, k_limb0_rows
@pytest.mark.parametrize("name", ALL_CHAINS)
@pytest.mark.parametrize("n", [1024, 64])
def test_rows(ctx, name, n):
    """three slots of q - 1, maximum halves and sprinkled extremes: pack equals the model's bytes and leaves the 16 bytes behind alone;
    unpack and limb0_rows (packed and dense) equal the dense words; unpack of pack is the identity"""
    X = ctx(name, n)
    rng = np.random.default_rng([n, len(name)])
    dense = np.stack([ev.fill_poly(f, X.qs, n, rng) for f in ("q-1", "max_halves", "sprinkled")])
    want = X.rows.words(dense)
    got = X.step("pack_rows", [dense], np.full(want.size + 2, M.PATTERN, dtype=np.uint64), batch=3)
    assert (got[:-2] == want).all() and (got[-2:] == M.PATTERN).all()
    back = X.step("unpack_rows", [want], np.full(dense.shape, M.PATTERN, dtype=np.uint64), batch=3)
    assert (back == dense).all()
    assert (X.step("unpack_rows", [np.ascontiguousarray(got[:-2])], np.full(dense.shape, M.PATTERN, dtype=np.uint64), batch=3) == dense).all()
    for packed, src in ((1, want), (0, dense)) if X.any_packed else ((0, dense),):       # (rows of 64 bits alone: PACKED is refused, test_refusals)
        limb0 = X.step("limb0_rows", [src], np.full((3, n), M.PATTERN, dtype=np.uint64), flags=STEP_PACKED if packed else 0, batch=3)
        assert (limb0 == dense[:, 0]).all(), packed


# ================================================================ refusals
def test_refusals(ctx):
    """one case per refusal of include/apsu_he.h: ValueError with its reason, nothing launched (the output keeps its pattern)"""
    X, W = ctx("mixed", 64), ctx("60x3", 64)
    n, L = 64, X.L
    case = M.make_case("refusal", X.qs, n, [(0, L, 2, 2)], 1, table=False)

    def refused(Y, why, step, ins, out, **kw):
        before = out.copy()
        with pytest.raises(ValueError, match=why):
            Y.step(step, ins, out, **kw)
        assert (out == before).all()

    def mac_args(c, **kw):
        return dict(dict(terms=c.terms, polys=c.polys, batch=c.batch, e0=0, n_ext=c.NL), **kw)

    dense, packed = case.coeffs, X.slots(case.coeffs, 1)
    # a word that is not canonical, in either operand and either format
    bad = case.powers.copy(); bad[0, 1, 1, 2, 5] = X.qs[2]
    refused(X, "powers.*canonical", "mac", [bad, dense, None], case.out0(), **mac_args(case))
    bad = dense.copy(); bad[0, 1, 0, 3, 63] = X.qs[3]
    refused(X, "plaintexts.*canonical", "mac", [case.powers, bad, None], case.out0(), **mac_args(case))
    bad = dense.copy(); bad[0, 1, 0, 0, 63] = X.qs[0]                       # 33 bits like its modulus: it packs, and decodes to q
    refused(X, "bit-packed plaintexts.*canonical", "mac", [case.powers, X.slots(bad, 1), None], case.out0(), **mac_args(case, flags=STEP_PACKED))
    # the three-product form where a prime does not admit it; packed where every row is 64 bits wide
    wcase = M.make_case("refusal", W.qs, n, [(0, W.L, 1, 2)], 2, table=False)
    refused(W, "mac_kara_usable", "mac", [wcase.powers, wcase.coeffs, None], wcase.out0(), **mac_args(wcase, flags=STEP_KARA))
    refused(W, "64 bits wide", "mac", [wcase.powers, wcase.coeffs, None], wcase.out0(), **mac_args(wcase, flags=STEP_PACKED))
    # limbs beyond the level, streams outside 1 .. 4, a chain of no terms
    refused(X, "beyond the level", "mac", [case.powers, dense, None], case.out0(), **mac_args(case, e0=1))
    refused(X, "beyond the level", "mac", [case.powers, dense, None], np.full((1, 2, 2, L + 1, n), M.PATTERN, dtype=np.uint64), **mac_args(case, n_ext=L + 1))
    refused(X, "outside 1 .. 4", "mac", [case.powers, dense, None], case.out0(), **mac_args(case, polys=0))
    refused(X, "outside 1 .. 4", "mac", [case.powers, dense, None], case.out0(), **mac_args(case, polys=5))
    refused(X, "no terms", "mac", [case.powers, dense, None], case.out0(), **mac_args(case, terms=0))
    for entry, why in (((1, L, 2, 2), "beyond the level"), ((0, L, 3, 2), "streams"), ((0, L, 2, 0), "no terms"), ((0, L, 2, 3), "longer than terms")):
        refused(X, why, "mac", [case.powers, dense, np.array([entry], dtype=np.uint64)], case.out0(), **mac_args(case))
    refused(X, "wrong size", "mac", [case.powers, packed, None], case.out0(), **mac_args(case))                # packed words without the flag
    # term_product
    T = M.TermCase(X.qs, n, 1, batch=2, repeat=2, seed=3)
    targs = dict(terms=T.repeat, batch=T.batch)
    refused(X, "beyond the level", "term_product", [T.powers, T.coeffs], T.out0(), e0=L, **targs)
    bad = T.powers.copy(); bad[1, 1, 1, 0] = X.qs[1]
    refused(X, "powers.*canonical", "term_product", [bad, T.coeffs], T.out0(), e0=1, **targs)
    bad = T.coeffs.copy(); bad[1, 2, 7] = X.qs[2]
    refused(X, "plaintexts.*canonical", "term_product", [T.powers, bad], T.out0(), e0=1, **targs)
    refused(X, "wrong size", "term_product", [T.powers, T.coeffs], T.out0()[:-1], e0=1, **targs)               # no guard behind the last job
    # the rows
    one = np.stack([ev.fill_poly("q-1", X.qs, n)])
    bad = one.copy(); bad[0, 1, 0] = X.qs[1]
    refused(X, "canonical", "pack_rows", [bad], np.full(X.rows.slot_bytes // 8 + 2, M.PATTERN, dtype=np.uint64), batch=1)
    tiny = np.zeros(8, dtype=np.uint64)
    refused(X, "65535 rows", "pack_rows", [tiny], tiny.copy(), batch=65535 // L + 1)
    refused(X, "65535 rows", "unpack_rows", [tiny], tiny.copy(), batch=65535 // L + 1)
    refused(W, "64 bits wide", "limb0_rows", [wcase.coeffs[0, 0]], np.full((2, n), M.PATTERN, dtype=np.uint64), flags=STEP_PACKED, batch=2)
