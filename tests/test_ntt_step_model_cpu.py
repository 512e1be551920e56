"""CPU tier of the transform steps: tests/ntt_step_model.py held to four references, and the table of launches of the GPU test held
to the kernels' form tables.

  the definition   out[i] = a(psi^(2 brv(i) + 1)): complete at n <= 256 (oracle/pymodel.py Model.ntt), Horner at sampled indices above
  the C oracle     transform_to_ntt / transform_from_ntt on the data primes of the GPU test's contexts, every ring size
  the emulation    emu_ntt_limb, emu_ntt_limb_c, emu_ntt_limb_ex and emu_intt_tensor_limb_c (apsu_amd/csrc/emu/ntt.cpp: the pass functions
                   the kernels run, RED 0 / 1 / 2, RAW on and off, both per-lane forms) on every directed case of the GPU test that fits
                   one limb: the fills, the reduced-gather edges, the unreduced gather at its boundary, the solved lazy operands, the RAW
                   bound and congruence
  emu_reduce128    the fold, canonical and lazy, for the fold word
"""
import ctypes as C

import numpy as np
import pytest

import emu_lib
from emu_lib import vp
import ntt_step_model as M
from oracle import pymodel, ref

EMU_LOGNS = [l for l in M.LOGNS if l < M.SPLIT_LOGN]
# a wide-near modulus per ring: a 61-bit prime behind the ones an emulation context takes for its own auxiliary base
SEAL61 = {logn: pymodel.get_primes(2 << logn, 61, 8)[-1] for logn in EMU_LOGNS}


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


def moduli(logn):
    return M.context_primes(logn) + [SEAL61[logn]]


def forms(logn):
    """(threads, coeffs per lane) of both per-lane forms"""
    n = 1 << logn
    return [(max(64, n // 16), 16)] + ([(n // 8, 8)] if logn in M.PLAN8 else [])


def emu_ex(emu, logn, m, data, inverse=False, src=None, red=0, raw=False, form=None):
    T, c = form or forms(logn)[0]
    out = np.ascontiguousarray(data, dtype=np.uint64).copy()
    s = np.ascontiguousarray(src, dtype=np.uint64) if src is not None else None
    rc = emu.emu_ntt_limb_ex(logn, int(inverse), C.c_uint64(m), vp(s) if s is not None else None, vp(out), T, c, red, int(raw))
    assert rc == 0, emu.emu_last_error()
    return out


def emu_tensor(emu, logn, m, ops, lazy, raw, form):
    T, c = form
    a0, a1, b0, b1 = (np.ascontiguousarray(x, dtype=np.uint64) for x in ops)
    outs = []
    for x0, y0, x1, y1 in ((a0, b0, None, None), (a0, b1, a1, b0), (a1, b1, None, None)):
        out = np.zeros(1 << logn, dtype=np.uint64)
        rc = emu.emu_intt_tensor_limb_c(logn, C.c_uint64(m), vp(x0), vp(y0), vp(x1) if x1 is not None else None, vp(y1) if y1 is not None else None,
                                        vp(out), T, c | (0x100 if lazy else 0) | (0x200 if raw else 0))
        assert rc == 0, (rc, emu.emu_last_error())
        outs.append(out)
    return outs


# ---------------------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("logn", [6, 8])
def test_model_is_the_definition_complete(logn):
    n = 1 << logn
    for m in moduli(logn):
        P = pymodel.Model(n, [m], M.T_PLAIN)
        a = [int(v) for v in M.canonical_fill("sprinkled", m, n)]
        f = [int(v) for v in M.forward(a, m, logn)]
        assert f == P.ntt(a, m)
        assert [int(v) for v in M.inverse(f, m, logn)] == a == P.intt(f, m)


@pytest.mark.parametrize("logn", [10, 11, 12, 13, 14, 15])
def test_model_is_the_definition_at_sampled_outputs(logn):
    n = 1 << logn
    for m in M.context_primes(logn)[:3]:
        a = M.canonical_fill("sprinkled", m, n)
        f = M.forward(a, m, logn)
        for i in (0, 1, 2, n // 2 - 1, n // 2, n - 2, n - 1, 0x2AAA % n, 0x1555 % n):
            assert int(f[i]) == M.evaluate_at(a, m, logn, i)
        assert (M.inverse(f, m, logn) == M.O(a)).all()


def test_raw_reading_undoes_the_twist():
    logn, m = 8, M.context_primes(8)[0]
    n = 1 << logn
    x = M.O(M.canonical_fill("alternating", m, n))
    psi = M.roots(m, logn)[0]
    words = x * n * np.array([pow(psi, k, m) for k in range(n)], dtype=object) % m + m        # any representative of x n psi^k
    assert (M.raw_residue(words, m, logn) == x).all()


# ---------------------------------------------------------------------------------------------------------------- the C oracle
@pytest.mark.parametrize("logn", M.LOGNS)
def test_model_against_the_c_oracle(logn):
    n = 1 << logn
    q = M.context_primes(logn)
    R = ref.RefContext(n, coeff_modulus=q, plain_modulus=M.T_PLAIN)
    lvl = len(q) - 2
    for fill in (("sprinkled", "q-1") if logn >= 14 else M.FILLS):
        x = np.stack([M.canonical_fill(fill, q[j], n) for j in range(lvl + 1)])[None]
        y = x.copy()
        R.transform_to_ntt(y, lvl)
        z = x.copy()
        R.transform_from_ntt(z, lvl)
        for j in range(lvl + 1):
            assert (y[0, j] == M.U(M.forward(x[0, j], q[j], logn))).all(), (logn, fill, j)
            assert (z[0, j] == M.U(M.inverse(x[0, j], q[j], logn))).all(), (logn, fill, j)


# ---------------------------------------------------------------------------------------------------------------- the fold word
def test_fold_word_against_the_emulation(emu):
    emu.emu_reduce128_lazy.argtypes = [C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    for logn in (12, 13):
        for m in moduli(logn):
            if not M.fold128_ok(m):
                assert emu.emu_reduce128_lazy(m, logn, None, None, None, 0) == 0
                continue
            quads = M.tensor_quads(m) + [tuple(int(v) for v in r) for r in np.random.default_rng(m % 1000).integers(0, m, (200, 4), dtype=np.uint64)]
            P = [x0 * y0 + x1 * y1 for x0, y0, x1, y1 in quads]
            hi = np.array([p >> 64 for p in P], dtype=np.uint64)
            lo = np.array([p & (M.W64 - 1) for p in P], dtype=np.uint64)
            out = np.zeros(len(P) + 2, dtype=np.uint64)
            assert emu.emu_reduce128_lazy(m, logn, vp(hi), vp(lo), vp(out), len(P)) == M.fold_params(m)[0]
            assert [int(v) for v in out[:len(P)]] == [M.reduce128_lazy(p, m) for p in P]
            assert int(out[-2]) == M.lazy_bound_q(m) and bool(out[-1]) == M.lazy_input_ok(m, logn)
            assert max(int(v) for v in out[:len(P)]) < M.lazy_bound_q(m) * m
            canon = np.zeros(len(P), dtype=np.uint64)
            assert emu.emu_reduce128(C.c_uint64(m), vp(hi), vp(lo), vp(canon), len(P)) == M.fold_params(m)[0]
            assert [int(v) for v in canon] == [p % m for p in P]


def context_moduli(logn, narrow_aux):
    """the 13 moduli of the GPU test's context of this ring, as the engine's parameter code picks them (emu_device_constants): the five
    coefficient primes, the seven auxiliary primes of the narrow or of SEAL's base, the plain modulus"""
    emu = emu_lib.load()
    lay = np.zeros(5, dtype=np.uint64)
    emu.emu_dev_layout(vp(lay))
    step = int(lay[0]) * (2 if logn == M.SPLIT_LOGN else 1)
    q = np.array(M.context_primes(logn), dtype=np.uint64)
    buf = np.zeros(1 << 16, dtype=np.uint8)
    nb = emu.emu_device_constants(None, C.c_uint64(1 << logn), vp(q), len(q), C.c_uint64(M.T_PLAIN), int(narrow_aux), b"tabs", vp(buf), C.c_uint64(buf.size))
    assert 0 < nb <= buf.size, emu.emu_last_error()
    return [int(buf[i * step:i * step + 8].view(np.uint64)[0]) for i in range(nb // step)]


def lazy_moduli():
    """every modulus a tensor launch of the GPU test can meet that takes lazy input: coefficient and auxiliary primes of both bases"""
    found = {(m, logn) for logn in EMU_LOGNS for m in moduli(logn) if M.lazy_input_ok(m, logn)}
    for logn in EMU_LOGNS:
        for narrow_aux in (True, False):
            found |= {(m, logn) for m in context_moduli(logn, narrow_aux) if M.lazy_input_ok(m, logn)}
    return sorted(found)


def test_contexts_of_the_gpu_test_hold_the_moduli_it_expects():
    for logn in M.LOGNS:
        for narrow_aux in (True, False):
            mods = context_moduli(logn, narrow_aux)
            assert len(mods) == 13 and mods[:5] == M.context_primes(logn) and mods[12] == M.T_PLAIN
            assert {M.mod_class(m, logn) for m in mods[5:12]} == ({"narrow"} if narrow_aux else {"wide_near"})


@pytest.mark.parametrize("m,logn", lazy_moduli(), ids=lambda v: hex(v) if v > 64 else "logn%d" % v)
def test_solved_operands_reach_past_the_fills_and_random_draws(m, logn):
    """Numbers, conditions 1 and 2, for the coefficient AND the auxiliary primes: above all-(q - 1) and above 20 000 random quadruples;
    above 5 q on the 50-bit primes with a large c"""
    reached = max(M.largest_fold_word(m, *M.tensor_operands(layout, m, 64)) for layout in M.TENSOR_LAYOUTS)
    assert reached == M.fold_word(M.tensor_quads(m)[0], m)
    assert reached > M.fold_word((m - 1,) * 4, m) and reached > M.random_fold_max(m)
    if m.bit_length() == 50:
        assert reached > 5 * m
    assert all(0 <= v < m for quad in M.tensor_quads(m) for v in quad)


# ---------------------------------------------------------------------------------------------------------------- the emulation
@pytest.mark.parametrize("logn", EMU_LOGNS)
def test_fills_through_every_emulation_entry(emu, logn):
    """forward, inverse and RAW inverse of every fill, every modulus class, both per-lane forms; the old entries agree with the new"""
    n = 1 << logn
    for m in moduli(logn):
        for fill in (M.FILLS if logn <= 13 else ("q-1", "sprinkled")):
            x = M.canonical_fill(fill, m, n)
            fwd, inv = M.U(M.forward(x, m, logn)), M.U(M.inverse(x, m, logn))
            for form in forms(logn):
                assert (emu_ex(emu, logn, m, x, form=form) == fwd).all(), (hex(m), fill, form)
                assert (emu_ex(emu, logn, m, x, inverse=True, form=form) == inv).all(), (hex(m), fill, form)
                raw = emu_ex(emu, logn, m, x, inverse=True, raw=True, form=form)
                assert (M.U(M.raw_residue(raw, m, logn)) == inv).all(), (hex(m), fill, form)
                assert int(raw.max()) < M.raw_bound(m, logn), (hex(m), fill, form, int(raw.max()) / m)
                old = x.copy()
                assert emu.emu_ntt_limb_c(logn, 0, C.c_uint64(m), vp(old), form[0], form[1]) == 0 and (old == fwd).all()
                old = x.copy()
                assert emu.emu_ntt_limb_c(logn, 1, C.c_uint64(m), vp(old), form[0], form[1]) == 0 and (old == inv).all()
            old = x.copy()
            assert emu.emu_ntt_limb(logn, 0, C.c_uint64(m), vp(old), forms(logn)[0][0]) == 0 and (old == fwd).all()


@pytest.mark.parametrize("logn", EMU_LOGNS)
def test_reduced_gather_edges_through_the_emulation(emu, logn):
    mods = moduli(logn)
    src = M.reduced_sources(mods, logn)
    for j, m in enumerate(mods):
        for s in (src[j], src[(j + 1) % len(mods)]):
            want = M.U(M.gather(s, m, logn))
            for form in forms(logn):
                assert (emu_ex(emu, logn, m, np.zeros_like(s), src=s, red=1, form=form) == want).all(), (hex(m), form)


@pytest.mark.parametrize("logn", EMU_LOGNS)
def test_unreduced_gather_at_its_boundary_through_the_emulation(emu, logn):
    """every source word max_src - 1 with max_src + 4 logn q = 2^64 for the widest narrow modulus: RED = 2 gives the model's bits, and RED = 1's"""
    n = 1 << logn
    narrow = [m for m in moduli(logn) if M.is_narrow(m, logn)]
    max_src = M.nored_max_src(narrow, logn)
    assert M.gather_nored_ok(max(narrow), max_src, logn) and not M.gather_nored_ok(max(narrow), max_src + 1, logn)
    for kind in M.NORED_FILLS:
        s = M.nored_source(kind, max_src, n)
        assert int(s.max()) == max_src - 1
        for m in narrow:
            want = M.U(M.gather(s, m, logn))
            for form in forms(logn):
                assert (emu_ex(emu, logn, m, np.zeros_like(s), src=s, red=2, form=form) == want).all(), (hex(m), kind, form)
                assert (emu_ex(emu, logn, m, np.zeros_like(s), src=s, red=1, form=form) == want).all(), (hex(m), kind, form)
    wide = moduli(logn)[0]
    assert emu.emu_ntt_limb_ex(logn, 0, C.c_uint64(wide), vp(s), vp(np.zeros_like(s)), forms(logn)[0][0], 16, 2, 0) == -1


@pytest.mark.parametrize("logn", EMU_LOGNS)
def test_solved_operands_through_the_tensor_emulation(emu, logn):
    """the tensor loader on the solved quadruples: lazy where the modulus takes lazy input, canonical otherwise and for comparison;
    twisted and RAW, the RAW words under the bound of device.h for a lazy source"""
    n = 1 << logn
    for m in moduli(logn):
        if not M.fold128_ok(m):                                     # the emulation entry has the fold's moduli only (the engine's canonical path: barrett128)
            continue
        lazy_ok = M.lazy_input_ok(m, logn)
        for layout in (M.TENSOR_LAYOUTS if logn <= 12 else ("solved", "rotated")):
            ops = M.tensor_operands(layout, m, n)
            want = [M.U(w) for w in M.intt_tensor(*ops, m, logn)]
            for form in forms(logn):
                for lazy in ((False, True) if lazy_ok else (False,)):
                    got = emu_tensor(emu, logn, m, ops, lazy, False, form)
                    raw = emu_tensor(emu, logn, m, ops, lazy, True, form)
                    for p in range(3):
                        assert (got[p] == want[p]).all(), (hex(m), layout, form, lazy, p)
                        assert (M.U(M.raw_residue(raw[p], m, logn)) == want[p]).all(), (hex(m), layout, form, lazy, p)
                        assert int(raw[p].max()) < M.raw_bound(m, logn, lazy_source=lazy), (hex(m), layout, form, lazy, p, int(raw[p].max()) / m)


# ---------------------------------------------------------------------------------------------------------------- every kernel has run
EXPECTED_ROWS = sorted(
    [("k_ntt", logn, t, c, w, d) for logn, t, c, w in [(14, 1024, 16, 4), (13, 1024, 8, 4), (12, 512, 8, 4), (13, 512, 16, 4), (12, 256, 16, 4), (11, 128, 16, 4),
                                                        (10, 64, 16, 4), (8, 64, 16, 4), (6, 64, 16, 4)] for d in ("forward", "inverse")] +
    [("k_ntt", 13, 1024, 8, 8, "forward")] +
    [("k_ntt_gather", logn, t, c, w, "forward") for logn, t, c, w in [(13, 1024, 8, 4), (12, 512, 8, 4), (13, 1024, 8, 8), (14, 1024, 16, 4), (13, 512, 16, 4),
                                                                       (12, 256, 16, 4), (11, 128, 16, 4), (10, 64, 16, 4), (8, 64, 16, 4), (6, 64, 16, 4)]] +
    [("k_intt_tensor", logn, t, c, 4, "inverse") for logn, t, c in [(13, 1024, 8), (12, 512, 8), (14, 1024, 16), (13, 512, 16), (12, 256, 16), (11, 128, 16),
                                                                     (10, 64, 16), (8, 64, 16), (6, 64, 16)]] +
    # the two stage kernels of n = 32768: the first stage with and without its gather, the last stage
    [("k_ntt_first_stage", 15, 0, 0, 0, "forward"), ("k_ntt_first_stage", 15, 0, 0, 0, "gather"), ("k_ntt_last_stage", 15, 0, 0, 0, "inverse")])


def test_the_launch_table_reaches_every_kernel(emu):
    """ntt_form (through emu_ntt_form) over the launches the GPU test issues: their union is every row of k_ntt_forms (19 kernels),
    k_ntt_gather_forms (10) and k_intt_tensor_forms (9) and the two stage kernels.  A row added to a form table without a launch in
    ntt_step_model.launches() fails here, on the CPU"""
    assert len(EXPECTED_ROWS) == 38 + 3 and sorted(M.form_rows()) == EXPECTED_ROWS
    emu.emu_ntt_form.argtypes = [C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
    ran = set()
    for row in M.launches():
        out = np.zeros(4, dtype=np.int32)
        lat = M.AUTO_LIMBS if row["latency"] is None else row["latency"]
        # (a tensor launch states no narrowness: launch_intt_tensor passes false)
        emu.emu_ntt_form(row["logn"], M.KIND[row["kind"]], row["limbs"], lat, int(row["narrow"] and row["kind"] != "tensor"), vp(out))
        assert out[0] > 0, row
        ran.update(M.kernels_of(row, tuple(int(v) for v in out)))
    assert sorted(ran) == EXPECTED_ROWS, (sorted(set(EXPECTED_ROWS) - ran), sorted(ran - set(EXPECTED_ROWS)))


def test_the_launch_table_runs_both_sides_of_each_switch_over():
    rows = M.launches()
    for logn, kind, limbs in ((13, "forward", 256), (13, "forward", 257), (13, "inverse", 257), (13, "gather", 257), (12, "inverse", 1024), (12, "inverse", 1025)):
        assert any(r["logn"] == logn and r["kind"] == kind and r["limbs"] == limbs and r["latency"] is None for r in rows), (logn, kind, limbs)
