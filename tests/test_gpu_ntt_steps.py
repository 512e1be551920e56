"""GPU tier: every transform launcher alone, one launch at a time, bit for bit against the integer model.

apsu_he_debug_run_step (the steps from ntt_info on, apsu_amd/csrc/engine_ntt_steps.cpp) puts chosen words in front of ONE call of
launch_ntt, launch_ntt_gather or launch_intt_tensor with the context's own tables, its own APSU_HE_NTT_LATENCY_LIMBS setting and a
limb-to-modulus map of the test's; tests/ntt_step_model.py states the same step on Python integers (held to the definition, the C
oracle and the CPU emulation by tests/test_ntt_step_model_cpu.py).  The launches come from ntt_step_model.launches(), the table the
CPU tier proves to reach every row of the kernels' form tables.  Contexts: one per ring size (64 .. 32768) with chosen primes -- a
60-bit wide prime, the two primes on either side of the narrow criterion, a 50-bit prime with a large c, a 30-bit prime -- once with
the narrow auxiliary base and once with SEAL's 61-bit one, at n = 4096 and 8192 under all three form settings.  No tolerance, nothing
skipped; a RAW word is held to the model by congruence and to the RAW bound of device.h for its class; every tensor launch of the
worst operands asserts, per modulus that takes lazy input, that its fold word lies above what fills and random draws produce.
"""
import numpy as np
import pytest

import apsu_amd
import ntt_step_model as M
from apsu_amd.engine import STEP_INVERSE, STEP_MAP_RAW, STEP_NORED

pytestmark = pytest.mark.gpu

ROWS = M.launches()
POISON = 0xEEEEEEEEEEEEEEEE
assert STEP_MAP_RAW == M.MAP_RAW


def rows_of(kind, case):
    return [r for r in ROWS if r["kind"] == kind and r["case"] == case]


def row_id(r):
    lat = "auto" if r["latency"] is None else "lat%d" % r["latency"]
    extra = "-%dx%d+%d" % (r["njobs"], r["tlimbs"], r["n_plain"]) if r["kind"] == "tensor" else ""
    return "n%d-%s-%s-%d%s%s" % (1 << r["logn"], r["aux"], lat, r["limbs"], "-narrow" if r["narrow"] else "", extra)


class Ctx:
    def __init__(self, logn, aux, latency, mp):
        self.logn, self.n = logn, 1 << logn
        if aux == "seal":
            mp.setenv("APSU_HE_AUX_BASE", "seal")
        if latency is not None:
            mp.setenv("APSU_HE_NTT_LATENCY_LIMBS", str(latency))
        try:
            self.G = apsu_amd.HeContext(n=self.n, coeff_modulus=M.context_primes(logn), plain_modulus=M.T_PLAIN)
        finally:
            mp.delenv("APSU_HE_AUX_BASE", raising=False)
            mp.delenv("APSU_HE_NTT_LATENCY_LIMBS", raising=False)
        out = np.zeros(64, dtype=np.uint64)
        self.G.debug_run_step("ntt_info", 0, outs=[out])
        v = [int(x) for x in out]
        assert v[0] == logn and v[1] == 5 and v[2] == 7 and v[3] == 1
        self.K, self.mods = v[1], v[4:4 + 13]
        assert self.mods[:5] == M.context_primes(logn) and self.mods[12] == M.T_PLAIN
        # the auxiliary base is what the context was made for: SEAL's 61-bit primes (wide-near) or the engine's narrow ones
        aux_class = {M.mod_class(m, logn) for m in self.mods[5:12]}
        assert aux_class == ({"wide_near"} if aux == "seal" else {"narrow"}), (aux, aux_class)

    def all_ids(self):
        """the map of an 'all' launch: every modulus of the context; a handful at the two largest rings"""
        return [0, 1, 2, 3, self.K] if self.logn >= 14 else list(range(13))

    def narrow_ids(self):
        return [i for i in range(13) if M.is_narrow(self.mods[i], self.logn)]

    def narrow_stated(self, ids):
        return all(M.is_narrow(self.mods[i & (M.MAP_RAW - 1)], self.logn) for i in ids)

    def ntt(self, data, ids, inverse):
        out = np.zeros_like(data)
        self.G.debug_run_step("ntt", 0, ins=[data, np.array(ids, dtype=np.uint64)], outs=[out], flags=STEP_INVERSE if inverse else 0)
        return out

    def gather(self, src, idx, ids, nored=False, max_src=None):
        out = np.zeros((len(idx), self.n), dtype=np.uint64)
        ins = [src, np.array(idx, dtype=np.uint64), np.array(ids, dtype=np.uint64)]
        if max_src is not None:
            ins.append(np.array([max_src], dtype=np.uint64))
        self.G.debug_run_step("ntt_gather", 0, ins=ins, outs=[out], flags=STEP_NORED if nored else 0)
        return out

    def tensor(self, a, b, plain, ids, njobs, limbs, stride, dgap=0):
        """-> out [njobs][dgap or 3 limbs][n], poisoned beforehand: the words behind a job's [3][limbs][n] must come back as they went"""
        out = np.full((njobs, dgap or 3 * limbs, self.n), POISON, dtype=np.uint64) if njobs else None
        pout = np.zeros_like(plain) if plain is not None else None
        self.G.debug_run_step("intt_tensor", 0, ins=[a, b, plain, np.array(ids, dtype=np.uint64)], outs=[out, pout], batch=njobs, terms=limbs, polys=stride,
                              e0=dgap)
        return out, pout


_CTX = {}


@pytest.fixture(scope="module")
def ctx():
    mp = pytest.MonkeyPatch()

    def get(row):
        key = (row["logn"], row["aux"], row["latency"])
        if key not in _CTX:
            _CTX[key] = Ctx(*key, mp)
        return _CTX[key]
    yield get
    for X in _CTX.values():
        X.G.close()
    _CTX.clear()
    mp.undo()


# ---------------------------------------------------------------------------------------------------------------- references, once
_REF = {}


def ref(kind, m, logn, fill):
    """forward / inverse transform of canonical_fill(fill, m): computed once, shared, never written"""
    key = (kind, m, logn, fill)
    if key not in _REF:
        x = M.canonical_fill(fill, m, 1 << logn)
        _REF[key] = M.U((M.forward if kind == "forward" else M.inverse)(x, m, logn))
        _REF[key].setflags(write=False)
    return _REF[key]


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.argwhere(got != want)
    assert not len(bad), "%s: %d words differ, first at %s: got %#x, want %#x" % (what, len(bad), tuple(bad[0]), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


def raw_ok(X, words, m, want, what, lazy_source=False):
    """a RAW limb two ways: congruent to the model's residue, and below the bound device.h states for its class (n = 32768: congruence)"""
    same(M.U(M.raw_residue(words, m, X.logn)), want, what + " (RAW, congruence)")
    if X.logn < M.SPLIT_LOGN:
        bound = M.raw_bound(m, X.logn, lazy_source)
        top = int(words.max())
        print("%s: largest RAW word %.3f m, bound %.3f m" % (what, top / m, bound / m))
        assert top < bound, "%s: RAW word %#x is not below the bound %#x of device.h" % (what, top, bound)


def check_ntt(X, row, ids, fill_of, what):
    """one launch_ntt over row['limbs'] limbs: limb g is fill_of(g) of its modulus, in the direction of the row"""
    inverse = row["kind"] == "inverse"
    assert X.narrow_stated(ids) == row["narrow"]
    count, period = row["limbs"], len(ids)
    data = np.stack([M.canonical_fill(fill_of(g), X.mods[ids[g % period] & (M.MAP_RAW - 1)], X.n) for g in range(min(count, 4 * period))])
    if count > len(data):                                             # a switch-over launch: the first limbs again (4 period is a multiple of period)
        data = np.ascontiguousarray(np.resize(data, (count, X.n)))
    out = X.ntt(data, ids, inverse)
    seen = {}
    for g in range(count):
        e = ids[g % period]
        m = X.mods[e & (M.MAP_RAW - 1)]
        want = ref(row["kind"], m, X.logn, fill_of(g))
        if e & M.MAP_RAW:
            key = (e, fill_of(g))
            if key in seen:                                           # the same words through the same kernel: the same bits
                same(out[g], out[seen[key]], "%s limb %d against limb %d" % (what, g, seen[key]))
            else:
                seen[key] = g
                raw_ok(X, out[g], m, want, "%s limb %d (modulus %#x)" % (what, g, m))
        else:
            same(out[g], want, "%s limb %d (modulus %#x)" % (what, g, m))


def inverse_map(ids):
    """every modulus twisted and RAW in one map"""
    return [v for i in ids for v in (i, i | M.MAP_RAW)]


# ---------------------------------------------------------------------------------------------------------------- NTT
@pytest.mark.parametrize("fill", M.FILLS)
@pytest.mark.parametrize("row", rows_of("forward", "all") + rows_of("inverse", "all"), ids=row_id)
def test_ntt_every_modulus_in_one_launch(ctx, row, fill):
    """every modulus of the context in one launch (narrow, wide and wide-near limbs together; inverse: RAW and twisted entries mixed),
    count no multiple of period"""
    X = ctx(row)
    ids = inverse_map(X.all_ids()) if row["kind"] == "inverse" else X.all_ids()
    assert row["limbs"] % len(ids) != 0
    check_ntt(X, row, ids, lambda g: fill, "%s %s" % (row["kind"], fill))


@pytest.mark.parametrize("row", rows_of("forward", "short") + rows_of("inverse", "short"), ids=row_id)
def test_ntt_count_below_period(ctx, row):
    X = ctx(row)
    ids = inverse_map(X.all_ids()) if row["kind"] == "inverse" else X.all_ids()
    ids = ids[1:] + ids[:1]                                           # (the wide-to-narrow order of the other test, rotated)
    assert row["limbs"] < len(ids)
    check_ntt(X, row, ids, lambda g: M.FILLS[g % 4], row["kind"] + " short")


@pytest.mark.parametrize("row", rows_of("forward", "switch") + rows_of("inverse", "switch"), ids=row_id)
def test_ntt_switch_overs(ctx, row):
    """256 | 257 limbs at n = 8192 and 1024 | 1025 at n = 4096 under the default selection: k_ntt<13, false, 1024, 8, 8> (narrow moduli
    only) and the inverse's 16-per-lane form above the switch"""
    X = ctx(row)
    ids = [1, 3, 4] if row["narrow"] else ([0, 1 | M.MAP_RAW, 2, 3 | M.MAP_RAW, 5] if row["kind"] == "inverse" else [0, 1, 2, 3, 5])
    check_ntt(X, row, ids, lambda g: M.FILLS[(g % (4 * len(ids))) // len(ids)], "%s %d limbs" % (row["kind"], row["limbs"]))


# ---------------------------------------------------------------------------------------------------------------- gather
def check_gather(X, src, idx, ids, out, what):
    memo = {}
    for g in range(len(idx)):
        m = X.mods[ids[g % len(ids)]]
        key = (idx[g], m)
        if key not in memo:
            memo[key] = M.U(M.gather(src[idx[g]], m, X.logn))
        same(out[g], memo[key], "%s limb %d (source %d, modulus %#x)" % (what, g, idx[g], m))


@pytest.mark.parametrize("row", rows_of("gather", "reduced") + rows_of("gather", "reduced-switch"), ids=row_id)
def test_gather_reduces_any_word(ctx, row):
    """sources 0, q - 1, q, 2q, 2^63, 2^64 - q, 2^64 - 1 of every target: each target reads its own edges and its neighbour's"""
    X = ctx(row)
    ids = X.all_ids() if row["case"] == "reduced" else [0, 1, 2, 3, 5]
    assert X.narrow_stated(ids) == row["narrow"]
    src = M.reduced_sources([X.mods[i] for i in ids], X.logn)
    idx = [(g + g // len(ids)) % len(ids) for g in range(row["limbs"])]
    check_gather(X, src, idx, ids, X.gather(src, idx, ids), "reduced gather")


@pytest.mark.parametrize("row", rows_of("gather", "nored") + rows_of("gather", "nored-switch"), ids=row_id)
def test_gather_unreduced_at_its_boundary(ctx, row):
    """max_src = 2^64 - 4 logn q of the widest narrow target, every source word max_src - 1 (then alternating with 0, then sprinkled): the
    boundary ntt_gather_nored_ok admits, from both sides -- one higher is refused, and the reducing launch gives the same bits"""
    X = ctx(row)
    ids = X.narrow_ids()
    assert 1 in ids and X.narrow_stated(ids) == row["narrow"]
    max_src = M.nored_max_src([X.mods[i] for i in ids], X.logn)
    assert all(M.gather_nored_ok(X.mods[i], max_src, X.logn) for i in ids) and not M.gather_nored_ok(X.mods[1], max_src + 1, X.logn)
    src = np.stack([M.nored_source(k, max_src, X.n) for k in M.NORED_FILLS])
    idx = [(g + g // len(ids)) % 3 for g in range(row["limbs"])]
    out = X.gather(src, idx, ids, nored=True, max_src=max_src)
    check_gather(X, src, idx, ids, out, "unreduced gather")
    same(X.gather(src, idx, ids), out, "the reducing launch")
    with pytest.raises(ValueError, match="ntt_gather_nored_ok"):
        X.gather(src, idx, ids, nored=True, max_src=max_src + 1)


# ---------------------------------------------------------------------------------------------------------------- tensor
_FED = {}


def fed_elsewhere(m):
    """what the other tests feed the loader, per modulus: the fold word of all-(q - 1) operands and the largest of 20 000 random quadruples"""
    if m not in _FED:
        _FED[m] = (M.fold_word((m - 1,) * 4, m), M.random_fold_max(m))
    return _FED[m]


def check_tensor(X, row, limb_ids, plain_ids, raw_of, layout, what):
    """one launch_intt_tensor; -> {modulus: the largest fold word its operands hand the transform} for the moduli that take lazy input"""
    njobs, limbs, n_plain, stride, dgap = row["njobs"], row["tlimbs"], row["n_plain"], row.get("stride", row["tlimbs"]), row.get("dgap", 0)
    reached = {}
    n = X.n
    a = np.zeros((njobs, 2, stride, n), dtype=np.uint64)
    b = np.zeros((njobs, 2, stride, n), dtype=np.uint64)
    ids = []
    for jb in range(njobs):
        for e in range(limbs):
            m = X.mods[limb_ids[e]]
            a[jb, 0, e], a[jb, 1, e], b[jb, 0, e], b[jb, 1, e] = M.tensor_operands(layout, m, n, shift=jb * limbs + e)
            if M.lazy_input_ok(m, X.logn):
                reached[m] = max(reached.get(m, 0), M.largest_fold_word(m, a[jb, 0, e], a[jb, 1, e], b[jb, 0, e], b[jb, 1, e]))
        for e in range(limbs, stride):                               # limbs the launch must not read: words no modulus admits
            a[jb, :, e] = b[jb, :, e] = M.W64 - 1
        ids += [limb_ids[e] | (M.MAP_RAW if raw_of(jb, p, e) else 0) for p in range(3) for e in range(limbs)]
    plain = None
    if n_plain:
        plain = np.stack([M.canonical_fill(M.FILLS[g % 4], X.mods[plain_ids[g] & (M.MAP_RAW - 1)], n) for g in range(n_plain)])
        ids += plain_ids[:n_plain]
    assert row["limbs"] == len(ids)
    out, pout = X.tensor(a, b, plain, ids, njobs, limbs, stride, dgap)
    if njobs:
        assert (out[:, 3 * limbs:] == POISON).all(), what + ": a word behind a job's output was written"
        out = out[:, :3 * limbs].reshape(njobs, 3, limbs, n)
    for jb in range(njobs):
        for e in range(limbs):
            m = X.mods[limb_ids[e]]
            want = M.intt_tensor(a[jb, 0, e], a[jb, 1, e], b[jb, 0, e], b[jb, 1, e], m, X.logn)
            for p in range(3):
                w = "%s job %d poly %d limb %d (modulus %#x)" % (what, jb, p, e, m)
                if raw_of(jb, p, e):
                    raw_ok(X, out[jb, p, e], m, M.U(want[p]), w, lazy_source=True)
                else:
                    same(out[jb, p, e], M.U(want[p]), w)
    for g in range(n_plain):
        m = X.mods[plain_ids[g] & (M.MAP_RAW - 1)]
        want = ref("inverse", m, X.logn, M.FILLS[g % 4])
        if plain_ids[g] & M.MAP_RAW:
            raw_ok(X, pout[g], m, want, "%s plain limb %d" % (what, g))
        else:
            same(pout[g], want, "%s plain limb %d (modulus %#x)" % (what, g, m))
    return reached


@pytest.mark.parametrize("layout", M.TENSOR_LAYOUTS)
@pytest.mark.parametrize("row", rows_of("tensor", "operands"), ids=row_id)
def test_tensor_worst_operands(ctx, row, layout):
    """every modulus of the context in one launch, RAW and twisted outputs mixed: the solved quadruples at every coefficient, rotated,
    sprinkled, and q - 1; a modulus that takes no lazy input runs the same operands through the canonical path"""
    X = ctx(row)
    reached = check_tensor(X, row, X.all_ids(), [], lambda jb, p, e: (p + e) % 2 == 1, layout, "tensor " + layout)
    # Every modulus of the launch that takes lazy input, the auxiliary primes included, on the operands just launched: the solved,
    # rotated and sprinkled layouts hand the transform a fold word strictly above what all-(q - 1) operands and 20 000 random quadruples
    # produce, and above 5 q on the 50-bit primes with a large c (a bound of 5 is violated by this input); the q-1 layout is that fill.
    assert set(reached) == {X.mods[i] for i in X.all_ids() if M.lazy_input_ok(X.mods[i], X.logn)} and reached
    for m, w in sorted(reached.items()):
        fill_word, random_word = fed_elsewhere(m)
        print("modulus %#x (%s): fold word %.5f q; all-(q - 1) %.5f q, random %.5f q, ntt_lazy_bound_q %d" % (m, layout, w / m, fill_word / m, random_word / m, M.lazy_bound_q(m)))
        assert w < M.lazy_bound_q(m) * m
        if layout == "q-1":                                             # (the fill the others are compared with)
            continue
        assert w > fill_word and w > random_word, "modulus %#x: the operands reach no further than the other tests' input" % m
        if m.bit_length() == 50:
            assert w > 5 * m


@pytest.mark.parametrize("row", rows_of("tensor", "shape"), ids=row_id)
def test_tensor_launch_shapes(ctx, row):
    """pairs % 8 in {1, 7, 0} and one above 8 (the XCD-aware order pads to blocks of eight pairs), n_plain 0 and 3 joining the launch,
    RAW and twisted limbs mixed, the operands' polynomials further apart than the limb count and the jobs' outputs further apart than
    three limbs (src_ps and job.d differ from limbs * n; the words in between are poisoned and must come back untouched)"""
    X = ctx(row)
    pairs = row["njobs"] * row["tlimbs"]
    assert row["logn"] >= 14 or pairs in (1, 7, 8, 15)
    limb_ids = [3, 0, 5, 1, 2, 4, 6][:row["tlimbs"]]
    check_tensor(X, row, limb_ids, [3, 5 | M.MAP_RAW, 0], lambda jb, p, e: (jb + p + e) % 3 == 0, "sprinkled", "tensor %dx%d+%d" % (row["njobs"], row["tlimbs"], row["n_plain"]))


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(ctx):
    """one per rule of the step; nothing is launched, and the context works afterwards"""
    X = ctx(dict(logn=10, aux="narrow", latency=None))
    n, q = X.n, X.mods
    ok = np.stack([M.canonical_fill("sprinkled", q[i], n) for i in (0, 1)])
    with pytest.raises(ValueError, match="out of range"):
        X.ntt(ok, [0, 13], False)
    with pytest.raises(ValueError, match="forward"):
        X.ntt(ok, [0, 1 | M.MAP_RAW], False)
    with pytest.raises(ValueError, match="forward"):
        X.gather(ok, [0, 1], [0, 1 | M.MAP_RAW])
    bad = ok.copy()
    bad[1, n - 1] = q[1]
    with pytest.raises(ValueError, match="canonical"):
        X.ntt(bad, [0, 1], True)
    with pytest.raises(ValueError, match="wrong size"):
        X.G.debug_run_step("ntt", 0, ins=[ok, np.array([0, 1], dtype=np.uint64)], outs=[np.zeros(n, dtype=np.uint64)])
    with pytest.raises(ValueError, match="source index"):
        X.gather(ok, [0, 2], [0, 1])
    max_src = M.nored_max_src([q[1]], X.logn)
    src = np.stack([M.nored_source("max", max_src, n)])
    with pytest.raises(ValueError, match="ntt_gather_nored_ok"):         # a wide target
        X.gather(src, [0], [0], nored=True, max_src=max_src)
    with pytest.raises(ValueError, match="ntt_gather_nored_ok"):         # a pair one past the boundary
        X.gather(src, [0], [1], nored=True, max_src=max_src + 1)
    with pytest.raises(ValueError, match="below max_src"):
        X.gather(src, [0], [1], nored=True, max_src=max_src - 1)
    a = np.stack([M.canonical_fill("sprinkled", q[1], n)] * 2).reshape(1, 2, 1, n)
    worse = a.copy()
    worse[0, 1, 0, 5] = q[1]
    with pytest.raises(ValueError, match="canonical"):
        X.tensor(a, worse, None, [1, 1, 1], 1, 1, 1)
    with pytest.raises(ValueError, match="different moduli"):
        X.tensor(a, a, None, [1, 3, 1], 1, 1, 1)
    with pytest.raises(ValueError, match="canonical"):
        X.tensor(a, a, bad[1:2], [1, 1, 1, 1], 1, 1, 1)
    with pytest.raises(ValueError, match="wrong size"):
        X.tensor(a, np.ascontiguousarray(a[:, :1]), None, [1, 1, 1], 1, 1, 1)
    Y = ctx(dict(logn=15, aux="narrow", latency=None))
    s15 = np.zeros((1, Y.n), dtype=np.uint64)
    with pytest.raises(ValueError, match="32768"):
        Y.gather(s15, [0], [1], nored=True, max_src=1)
    with pytest.raises(ValueError, match="32768"):
        Y.tensor(np.zeros((1, 2, 1, Y.n), dtype=np.uint64), np.zeros((1, 2, 1, Y.n), dtype=np.uint64), None, [1, 1, 1], 1, 1, 1)
    # and the same contexts still work
    same(X.ntt(ok, [0, 1], False), np.stack([ref("forward", q[i], X.logn, "sprinkled") for i in (0, 1)]), "after the refusals")
    same(X.gather(src, [0], [1], nored=True, max_src=max_src)[0], M.U(M.gather(src[0], q[1], X.logn)), "after the refusals, gather")
