"""CPU tier: the engine's own auxiliary BEHZ base (HeParams::Create with AuxBase::Narrow, params.cpp narrow_aux_base).

For every shipped parameter file and every level the base the engine takes is narrow and meets SEAL's size bound
32 + bits(t) + bits(Q) < bits(prod(B) m_sk) with SEAL's prime count, or it is SEAL's base and the library says why.  The bound,
the narrow criterion and the tensor loader's lazy-input bound are recomputed here from their definitions, and every new prime
runs the tensor-on-load inverse through the workgroup emulation with lazy and with canonical input."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import common
import emu_lib
from oracle import ref

u64p = C.POINTER(C.c_uint64)
PARAM_FILES = sorted(f[:-5] for f in os.listdir(common.PARAM_DIR) if f.endswith(".json"))


@pytest.fixture(scope="module")
def emu():
    lib = emu_lib.load()
    lib.emu_aux_base.argtypes = [C.c_char_p, C.c_int, u64p, C.c_int]
    return lib


def aux_base(emu, js, narrow):
    out = np.zeros(256, dtype=np.uint64)
    k = emu.emu_aux_base(js.encode(), narrow, out.ctypes.data_as(u64p), len(out))
    assert 0 < k <= len(out), emu.emu_last_error()
    v = [int(x) for x in out[:k]]
    chosen, bits, logn, nl = v[:4]
    levels, i = [], 4
    for _ in range(nl):
        L, nB, m_sk, gamma = v[i:i + 4]
        levels.append(dict(L=L, nB=nB, m_sk=m_sk, gamma=gamma, B=v[i + 4:i + 4 + nB]))
        i += 4 + nB
    return dict(narrow=bool(chosen), bits=bits, logn=logn, levels=levels, note=emu.emu_last_error().decode())


def is_narrow(q, logn):
    return q * (4 * logn + 1) < 2 ** 64


def plan_k_last(logn):
    """stages of the throughput form's first inverse pass (ntt_core.h plan_k for the last forward pass)"""
    return {14: 4, 13: 4, 12: 3, 11: 2, 10: 4, 8: 2, 6: 3}.get(logn, 0)


def lazy_input_ok(q, logn):
    """ntt_lazy_input_ok restated: the fold word bound of q = 2^k - c, doubled per product-free stage of the first inverse pass"""
    k = q.bit_length()
    c = 2 ** k - q
    if not (44 <= k <= 61 and c < 2 ** 24 and (2 ** (64 - k) + 2) * c <= 2 ** k):
        return False
    bound = 5 + (((c << 32) + 4 * c * c) >> (k - 1))
    kk = plan_k_last(logn)
    return q * ((bound << kk) + 4 * (logn - kk)) < 2 ** 64


def seal_nB(L, t_bits, q_bits):
    return L + (1 if 32 + t_bits + q_bits >= 61 * L + 61 else 0)


@pytest.mark.parametrize("name", PARAM_FILES)
def test_aux_base_narrow_and_bounded_at_every_level(emu, name):
    js = common.param_json(name)
    sp = json.loads(js)["seal_params"]
    n = sp["poly_modulus_degree"]
    rc = ref.RefContext(n, sp["coeff_modulus_bits"], sp.get("plain_modulus", 0), sp.get("plain_modulus_bits", 0))
    q, t = [int(x) for x in rc.q], int(rc.t)
    seal = aux_base(emu, js, 0)
    mine = aux_base(emu, js, 1)
    assert not seal["narrow"] and seal["bits"] == 61
    assert len(mine["levels"]) == len(seal["levels"])
    if not mine["narrow"]:
        # SEAL's base kept: the reason names the level and the bound
        assert "size bound" in mine["note"] or "narrow primes" in mine["note"], mine["note"]
        assert mine["levels"] == seal["levels"]
        return
    logn = mine["logn"]
    assert 2 ** logn == n
    t_bits = t.bit_length()
    seen = set()
    for lv, sv in zip(mine["levels"], seal["levels"]):
        L = lv["L"]
        q_bits = 1
        Q = 1
        for x in q[:L]:
            Q *= x
        q_bits = Q.bit_length()
        assert lv["nB"] == sv["nB"] == seal_nB(L, t_bits, q_bits), name          # SEAL's count, never one more
        prod = lv["m_sk"]
        for b in lv["B"]:
            prod *= b
        assert 32 + t_bits + q_bits < prod.bit_length(), (name, L)
        primes = [lv["m_sk"], lv["gamma"]] + lv["B"]
        assert len(set(primes)) == len(primes)
        for p in primes:
            assert p % (2 * n) == 1 and p not in q and p != t
            assert p.bit_length() == mine["bits"] and 2 ** mine["bits"] - p < 2 ** 24
            assert is_narrow(p, logn) and lazy_input_ok(p, logn), (name, hex(p))
            assert all(pow(w, p - 1, p) == 1 for w in (2, 3, 5, 7, 11, 13))
            seen.add(p)
    # the largest bit size that gives narrow primes with lazy tensor input: one bit more would not
    assert not (is_narrow(2 ** (mine["bits"] + 1) - 1, logn) and lazy_input_ok(2 ** (mine["bits"] + 1) - 2 * n + 1, logn))
    if n == 8192:
        assert mine["bits"] == 57


def _aux_primes(emu, n):
    out = set()
    for name in PARAM_FILES:
        js = common.param_json(name)
        if json.loads(js)["seal_params"]["poly_modulus_degree"] != n:
            continue
        b = aux_base(emu, js, 1)
        assert b["narrow"], (name, b["note"])
        for lv in b["levels"]:
            out.update([lv["m_sk"], lv["gamma"]] + lv["B"])
    return sorted(out)


@pytest.mark.parametrize("n", [2048, 4096, 8192])
def test_aux_primes_take_lazy_tensor_input_in_the_emulation(emu, n):
    """every new prime through the tensor-on-load inverse of the workgroup emulation, lazy input (the fold's last word) and canonical
    input, both forms of the workgroup where the ring size has two: the same canonical output, equal to the product's inverse transform"""
    logn = n.bit_length() - 1
    emu.emu_intt_tensor_limb_c.argtypes = [C.c_int, C.c_uint64, u64p, u64p, u64p, u64p, u64p, C.c_int, C.c_int]
    primes = _aux_primes(emu, n)
    assert primes
    for q in primes:
        rng = np.random.default_rng(q % 1000003)
        x0, y0, x1, y1 = (rng.integers(0, q, n, dtype=np.uint64) for _ in range(4))
        for a in (x0, y0, x1, y1):
            a[:32] = q - 1                                        # a whole first-pass group of extreme inputs
        ref_out = None
        for co in [16] + ([8] if n in (4096, 8192) else []):
            for lazy in (0, 0x100):
                out = np.zeros(n, dtype=np.uint64)
                rc = emu.emu_intt_tensor_limb_c(logn, q, x0.ctypes.data_as(u64p), y0.ctypes.data_as(u64p), x1.ctypes.data_as(u64p),
                                                y1.ctypes.data_as(u64p), out.ctypes.data_as(u64p), n // co, co | lazy)
                assert rc == 0, (hex(q), co, lazy, rc, emu.emu_last_error())   # -3 would mean: lazy input refused for this prime
                assert int(out.max()) < q
                if ref_out is None:
                    ref_out = out
                assert (out == ref_out).all(), (hex(q), co, lazy)
        prod = np.array([(int(a) * int(b) + int(u) * int(v)) % q for a, b, u, v in zip(x0, y0, x1, y1)], dtype=np.uint64)
        assert emu.emu_ntt_limb(logn, 1, C.c_uint64(q), prod.ctypes.data_as(u64p), n // 16) == 0
        assert (ref_out == prod).all(), hex(q)


def test_extension_launch_form_follows_the_base(emu):
    """ntt_form with the narrowness the engine now states for launches over the extended base q u Bsk: the 16M-4096 extension forward
    transform (6 840 limbs) takes the 8-wave build with the narrow base and the 16-coefficient form with SEAL's; narrowness does not
    change the inverse or the tensor-on-load forms, and launches of at most 256 limbs keep the latency form either way"""
    emu.emu_ntt_form.argtypes = [C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(C.c_int)]
    auto = 2 ** 64 - 1
    FWD, INV, GATHER, TENSOR = range(4)
    out = (C.c_int * 4)()

    def form(kind, limbs, narrow):
        emu.emu_ntt_form(13, kind, limbs, auto, narrow, out)
        return tuple(out)

    wide_ext = form(FWD, 6840, 0)
    assert wide_ext == (512, 16, 4, 0)
    assert form(FWD, 6840, 1) == (1024, 8, 8, 0)
    for kind in (INV, TENSOR):
        for limbs in (200, 3420, 6840):
            assert form(kind, limbs, 1) == form(kind, limbs, 0)
    assert form(FWD, 256, 1) == form(FWD, 256, 0) == (1024, 8, 4, 0)
    # the engine states narrowness of the extended base from the base it took (16M-4096: narrow data primes and narrow Bsk)
    b = aux_base(emu, common.param_json("16M-4096"), 1)
    assert b["narrow"] and all(is_narrow(p, 13) for lv in b["levels"] for p in [lv["m_sk"]] + lv["B"])
