"""CPU tier: tests/mac_step_model.py held to the CPU emulation of the multiply-accumulate family, on the cases the GPU tier runs.

The model's three parts (sums, the row rule, the packed layout) are written from their definitions; here each is compared with what
apsu_amd/csrc/mac_core.h computes when the emulation library steps the kernels' own lane functions: pack / unpack byte for byte, the
row rule prime by prime, and the chain sums of every MacCase / TermCase of the case generator -- the same generator, with the job
fields set the same way, as tests/test_gpu_mac_steps.py feeds to the gfx950 kernels.  So a case the GPU tier runs is known to be
one on which the kernels' text, compiled for the host, agrees with the model; and a mutant of mac_core.h can be judged here.  Every
comparison is exact."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import edge_values as ev
import emu_lib
import mac_step_model as M
from emu_lib import vp
from oracle import pymodel, ref
from test_dev_consts_cpu import block, layouts
from test_mac_core_cpu import MAC_G, MacJob, TermJob, rules, u32, u64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_CHAINS = list(M.CHAINS)


@pytest.fixture(scope="module")
def emu():
    lib = emu_lib.load()
    assert lib.emu_mac_job_bytes() == C.sizeof(MacJob) == 112
    lib.emu_device_constants.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_int, C.c_uint64, C.c_int, C.c_char_p, C.c_void_p, C.c_uint64]
    return lib


class EmuLevel:
    """the constants the emulation's level takes, from the model: the row widths are the model's (64 each for a dense run)"""

    def __init__(self, emu, qs, n, packed):
        self.qs, self.n = [int(q) for q in qs], n
        self.rows = M.Rows(qs, n, None if packed else [64] * len(qs))
        self.keep = (u64(self.qs), u32([ev.mac_shift(q) for q in qs]), u32([ev.mac_chunk(q) for q in qs]), u32([rules(emu, q)[2] for q in qs]), u32(self.rows.bits))

    def args(self):
        return (len(self.qs),) + tuple(vp(a) for a in self.keep) + (C.c_uint64(self.n),)


def kara_usable(qs):
    return all(ev.mac_chunk_kara(q) for q in qs)


def run_mac_emu(emu, case, kara, packed, limb_slow):
    """k_mac over the case's jobs, the job table set as Engine::debug_run_mac_step sets it; -> the output array.  The output lies in a
    larger PATTERN-filled buffer, which is checked: a store that leaves the array is seen, not suffered"""
    lv = EmuLevel(emu, case.qs, case.n, packed)
    n, L, P, NL, polys, terms = case.n, case.L, case.P, case.NL, case.polys, case.terms
    pt = lv.rows.words(case.coeffs.reshape(-1, L, n), pad=True) if packed else case.coeffs
    slot = lv.rows.slot_bytes
    assert slot == (sum(lv.rows.bits) * n // 8)
    size = case.out0().size
    buf = np.full(size + 2 * (P + L) * n, M.PATTERN, dtype=np.uint64)
    jobs = (MacJob * case.batch)()
    for b, (limb0, nl, ng, cnt) in enumerate(case.jobs):
        j = jobs[b]
        j.pw = case.powers.ctypes.data + b * terms * 2 * P * n * 8
        j.cnt, j.ng, j.limb0, j.nl, j.packed, j.pad = cnt, ng, limb0, nl, int(packed), 0
        j.pt_stride, j.pw_stride, j.pw_poly_stride, j.out_poly_stride = (slot if packed else slot // 8), 2 * P * n, P * n, NL * n
        for g in range(MAC_G):
            j.pt[g] = pt.ctypes.data + (b * polys + (g if g < ng else 0)) * terms * slot
            j.out[g] = buf.ctypes.data + (b * polys + (g if g < polys else 0)) * 2 * NL * n * 8
    rc = emu.emu_mac(*lv.args(), jobs, case.batch, int(kara), int(packed), int(limb_slow))
    assert rc == 0, emu.emu_last_error()
    assert (buf[size:] == M.PATTERN).all(), "%s: a store behind the output array" % case.name
    return buf[:size]


def forms(qs, packed_possible=True):
    """(three-product, packed, limb_slow) a level is run in"""
    return [(k, p, s) for k in ((0, 1) if kara_usable(qs) else (0,)) for p in ((0, 1) if packed_possible else (0,)) for s in (0, 1)]


def data_primes(name, n):
    q, _, L = M.chain(name, n)
    return q[:L]


# ================================================================ the layout
@pytest.mark.parametrize("name", ALL_CHAINS)
@pytest.mark.parametrize("n", [64, 1024])
def test_pack_is_emu_pack_rows_byte_for_byte_and_back(emu, name, n):
    qs = data_primes(name, n)
    rows = M.Rows(qs, n)
    assert rows.bits == M.STORED[name]
    L, slots = len(qs), 3
    rng = np.random.default_rng([n, len(name)])
    dense = np.stack([ev.fill_poly(f, qs, n, rng) for f in ("q-1", "max_halves", "sprinkled")])
    mine = rows.pack(dense)
    buf = np.full(slots * rows.slot_bytes + M.PAD, 0xA5, dtype=np.uint8)
    assert emu.emu_pack_rows(L, vp(u32(rows.bits)), C.c_uint64(n), vp(dense), vp(buf), C.c_uint64(rows.slot_bytes), C.c_uint64(slots), 0, None) == 0
    assert (buf[:-M.PAD] == mine).all() and (buf[-M.PAD:] == 0xA5).all()
    back = np.zeros_like(dense)
    assert emu.emu_pack_rows(L, vp(u32(rows.bits)), C.c_uint64(n), None, vp(buf), C.c_uint64(rows.slot_bytes), C.c_uint64(slots), 1, vp(back)) == 0
    assert (back == dense).all() and (rows.unpack(mine, slots) == dense).all()
    assert (rows.words(dense, pad=True).view(np.uint8)[:-M.PAD] == mine).all()


def test_mixed_rows_start_off_the_16_byte_grid_at_n_64():
    """the claim next to CHAINS: limb 1 and limb 2 of the mixed slot start 8 bytes past a multiple of 16 at n = 64; at n = 1024 no order can"""
    rows = M.Rows(data_primes("mixed", 64), 64)
    assert [o % 16 for o in rows.row_off[1:3]] == [8, 8]
    assert all(1024 * w // 8 % 16 == 0 for w in range(32, 65))


# ================================================================ the row rule
def all_parameter_primes():
    out = set()
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "params", "*.json"))):
        out |= set(ref.RefContext.from_params(ref.load_params(path)).q)
    return sorted(out)


def test_row_rule_is_packed_row_bits_and_its_windows_fit(emu):
    primes = all_parameter_primes() + [q for c in ALL_CHAINS for n in (64, 1024) for q in M.chain(c, n)[0]]
    primes += [pymodel.get_primes(2048, b, 1)[0] for b in range(20, 62)]
    assert len(primes) > 100 and {q.bit_length() for q in primes} >= set(range(20, 62))
    widths = set()
    for q in primes:
        w = M.row_bits(q)
        assert w == emu.emu_packed_row_bits(C.c_uint64(q)), q
        assert w == 64 or max(q.bit_length(), 32) <= w < 64
        widths.add(w)
    assert widths == set(range(32, 51)) | {52, 56, 64}
    for w in widths:
        assert M.windows_fit(w, 32768), w
    assert not M.windows_fit(51, 1024) and not M.windows_fit(55, 1024) and not M.windows_fit(57, 1024)      # the widths the rule passes over do not


def test_window_shifts_at_49_bits():
    """test_mac_core_cpu.py's claim, kept next to the n = 1024 cases that rely on it: one block of 256 lanes of a 49-bit row meets every
    even shift of the 16-byte window"""
    assert {(k // 2) * 2 * 49 % 32 for k in range(0, 512, 2)} == set(range(0, 32, 2))


# ================================================================ the chains are contexts, and their level blocks are the model's
@pytest.mark.parametrize("name", ALL_CHAINS)
@pytest.mark.parametrize("n", [64, 1024])
def test_chain_is_a_context_with_the_models_rows(emu, name, n):
    """what test_gpu_mac_steps.py's mac_info check asks of the device block, asked here of the block the engine would upload"""
    q, t, L = M.chain(name, n)
    levels = block(emu, dict(n=n, primes=q, t=t, aux="narrow"), "levels").view(layouts(emu)["level"])
    assert len(levels) == L
    lv = levels[L - 1]
    rows = M.Rows(q[:L], n)
    assert rows.bits == M.STORED[name]
    for j in range(L):
        s = ev.mac_shift(q[j])
        assert (int(lv["mac_shift"][j]), int(lv["mac_chunk"][j])) == (s, ev.mac_chunk(q[j]))
        assert ev.mac_chunk_kara(q[j]) in (0, int(lv["mac_chunk_k"][j]))
        assert (int(lv["mac_bits"][j]), int(lv["mac_row_off"][j]), int(lv["mac_mask_hi"][j])) == (rows.bits[j], rows.row_off[j], M.mask_hi(rows.bits[j], s))


# ================================================================ the sums, on the GPU tier's cases
@pytest.mark.parametrize("name", M.EQUAL_CHAINS + ["36-36-60", "mixed"])
@pytest.mark.parametrize("n", [1024, 64])
def test_worst_case_launches(emu, name, n):
    """chains around each chunk (or one long chain) and of 1, 2, 3 terms; 1, 3, 4 streams; every operand an extreme; both forms, dense
    and packed, both grid orders; two blocks of lanes (n = 1024) and less than one (n = 64)"""
    qs = data_primes(name, n)
    for case in M.worst_case_launches(qs, n, seed=len(name) + n):
        for kara, packed, limb_slow in forms(qs):
            out = run_mac_emu(emu, case, kara, packed, limb_slow)
            assert case.wrong(out) == [], "%s n %d %s: three-product %d packed %d limb_slow %d" % (name, n, case.name, kara, packed, limb_slow)


@pytest.mark.parametrize("name", M.DIRECTED_CHAINS)
@pytest.mark.parametrize("n", [1024, 64])
def test_directed_launches(emu, name, n):
    """limb0 != 0, nl below L, P above L, out_poly_stride = nl n, a table of jobs that differ: what a job does not own keeps its pattern"""
    qs = data_primes(name, n)
    cases = M.directed_launches(qs, n, seed=n)
    assert {(c.jobs[0][0], c.jobs[0][1], c.P) for c in cases if not c.table} == {(a, b, P) for a, b in M.limb_windows(len(qs)) for P in (len(qs), len(qs) + 3)}
    for case in cases:
        for kara, packed, limb_slow in forms(qs):
            out = run_mac_emu(emu, case, kara, packed, limb_slow)
            assert case.wrong(out) == [], "%s n %d %s: three-product %d packed %d limb_slow %d" % (name, n, case.name, kara, packed, limb_slow)
        untouched = case.expected() == M.PATTERN
        assert untouched.any() == (case.table or False)    # the table's jobs leave limbs and streams alone; the others own their whole output


def run_term_emu(emu, T, packed):
    lv = EmuLevel(emu, T.qs, T.n, packed)
    n, L, P = T.n, T.L, T.P
    pt = lv.rows.words(T.coeffs, pad=True) if packed else T.coeffs
    slot = lv.rows.slot_bytes
    out = T.out0()
    gy = min(T.njobs, 32768)
    slots = gy * ((T.njobs + gy - 1) // gy)                # the launch's y x z: the entries behind njobs are no jobs; one that ran would hit the guard
    tj = (TermJob * slots)()
    for u in range(slots):
        b = u % T.batch
        tj[u].pt, tj[u].pw = pt.ctypes.data + b * slot, T.powers.ctypes.data + b * 2 * P * n * 8
        tj[u].out = out.ctypes.data + min(u, T.njobs) * 2 * n * 8
    rc = emu.emu_term_product(*lv.args(), tj, C.c_uint64(T.njobs), T.limb, P * n, n, int(packed))
    assert rc == 0, emu.emu_last_error()
    return out


@pytest.mark.parametrize("name", ["mixed", "50x3", "56x4", "60x3"])
def test_term_product_is_the_model_and_a_chain_of_one_term(emu, name):
    for n in (1024, 64):
        qs = data_primes(name, n)
        for limb in range(len(qs)):
            T = M.TermCase(qs, n, limb, batch=3, repeat=2, seed=[n, limb], P=len(qs) + (limb % 2) * 3)
            chain_case = T.as_mac_case()
            for packed in (0, 1):
                out = run_term_emu(emu, T, packed)
                assert (out == T.expected()).all(), (name, n, limb, packed)
                mac = run_mac_emu(emu, chain_case, 0, packed, 1).reshape(T.batch, 2, n)
                assert (mac == out[:T.batch]).all() and chain_case.wrong(mac) == []


@pytest.mark.parametrize("packed", [0, 1])
def test_term_product_second_z_slab(emu, packed):
    """32 768 + 5 jobs over 3 operand sets at n = 64: the grid's y is 32 768, five jobs lie in the second z slab and 32 763 of its entries are none"""
    qs = data_primes("mixed", 64)
    T = M.TermCase(qs, 64, 1, batch=3, repeat=(32768 + 5) // 3 + 1, seed=7)
    assert T.njobs >= 32768 + 5 and T.njobs % 32768 >= 5
    out = run_term_emu(emu, T, packed)
    assert (out == T.expected()).all() and (out[-1] == M.PATTERN).all()


def test_pack_rows_grid_check(emu):
    """the host check in front of every launch_pack_rows / launch_unpack_rows (engine_bundles.cpp, the PACK_ROWS / UNPACK_ROWS steps):
    slots * L rows must fit grid dimension y.  Tested here only, through the emulation's launch of the two kernels, which asks the same
    function first: a refused launch is not launched"""
    qs, n = data_primes("56x4", 64), 64
    rows = M.Rows(qs, n)
    dense = np.stack([ev.fill_poly("q-1", qs, n)])
    buf = np.zeros(rows.slot_bytes + M.PAD, dtype=np.uint8)

    def launch(slots, L, unpack):
        return emu.emu_pack_rows(L, vp(u32(rows.bits)), C.c_uint64(n), vp(dense), vp(buf), C.c_uint64(rows.slot_bytes), C.c_uint64(slots), unpack, vp(dense))

    assert launch(1, 3, 0) == 0 and launch(1, 3, 1) == 0
    for slots, L in ((65536, 1), (8192, 8), (21846, 3), (1 << 62, 4), (1, 0)):
        for unpack in (0, 1):
            assert launch(slots, L, unpack) == -1 and b"65535 rows" in emu.emu_last_error(), (slots, L)
    for slots, L in ((65535, 1), (8191, 8), (21845, 3)):          # the largest launches that pass (asked of the rule's restatement, not launched)
        assert slots * L <= 65535 < (slots + 1) * L
