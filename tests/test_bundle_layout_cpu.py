"""CPU tier: where each coefficient of a stored BinBundle lives (apsu_amd/csrc/bundle_layout.h: bundle_layout), enumerated through
the CPU emulation library and held to a restatement, written here, of the rule of the BatchedPlaintextPolyn ctor
(bin_bundle.cpp:385-420) and of use_ps (receiver_osn.cpp:520-522), and to the invariants the engine's readers rely on: the runs
partition 1 .. degree, neighbours differ in kind, the slots of a kind count up with the degree, a_{i h} is slot i - 1 of its kind and
inner polynomial i of the evaluation starts at slot i * l of the NTT-form coefficients."""
import ctypes as C
import os

import numpy as np
import pytest

import common
import emu_lib
from oracle import ref

u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)
REFUSAL = "ps_low_degree == 1 leaves coefficient-form plaintexts that eval() cannot multiply"
ALL_PARAM_FILES = sorted(f[:-5] for f in os.listdir(common.PARAM_DIR) if f.endswith(".json"))


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


def restated(ps, degree, first_chain_idx):
    """bin_bundle.cpp:385-420: plaintexts at chain index min(first, 2 with Paterson-Stockmeyer, else 1); coefficient d is transformed to
    NTT form iff (!ps && d != 0) || (ps && d % (ps + 1) != 0); receiver_osn.cpp:520-522: use_ps = ps > 1 && ps < degree.  The engine
    packs each kind in ascending degree."""
    h = ps + 1
    out = dict(use_ps=ps > 1 and ps < degree, H=degree // h if ps else 0, r=degree % h if ps else 0,
               pt_level=min(first_chain_idx, 2 if ps else 1), kind=[0], slot=[0])
    held = {1: 0, 2: 0}
    for d in range(1, degree + 1):
        kind = 1 if (not ps and d != 0) or (ps and d % h != 0) else 2
        out["kind"].append(kind)
        out["slot"].append(held[kind])
        held[kind] += 1
    out["ntt_count"], out["lifted_count"] = held[1], held[2]
    return out


def layout(emu, ps, degree, first_chain_idx):
    """-> dict like restated()'s plus runs [(d0, count, kind, first_slot)], or None for a refused shape"""
    out = np.zeros(7 + 4 * (degree + 1), dtype=np.uint64)
    where = np.zeros(2 * (degree + 1), dtype=np.uint32)
    k = emu.emu_bundle_layout(ps, degree, first_chain_idx, out.ctypes.data_as(u64p), len(out), where.ctypes.data_as(u32p))
    if k < 0:
        assert emu.emu_last_error().decode() == REFUSAL
        return None
    v = [int(x) for x in out[:k]]
    assert k == 7 + 4 * v[6]
    return dict(use_ps=bool(v[0]), H=v[1], r=v[2], pt_level=v[3], ntt_count=v[4], lifted_count=v[5],
                runs=[tuple(v[7 + 4 * i:11 + 4 * i]) for i in range(v[6])], kind=[int(x) for x in where[0::2]], slot=[int(x) for x in where[1::2]])


def check(emu, ps, degree, first_chain_idx):
    y = layout(emu, ps, degree, first_chain_idx)
    if ps == 1 and degree >= 2:
        assert y is None, "ps_low_degree == 1 above degree 1 is refused"
        return
    assert y is not None
    want = restated(ps, degree, first_chain_idx)
    for name, value in want.items():
        assert y[name] == value, (ps, degree, first_chain_idx, name)
    # the runs partition 1 .. degree, are maximal, and name the slots where() names
    at = 1
    for i, (d0, count, kind, first_slot) in enumerate(y["runs"]):
        assert d0 == at and count >= 1 and kind in (1, 2)
        assert i == 0 or y["runs"][i - 1][2] != kind
        for j in range(count):
            assert (y["kind"][d0 + j], y["slot"][d0 + j]) == (kind, first_slot + j)
        at += count
    assert at == degree + 1
    for kind, held in ((1, y["ntt_count"]), (2, y["lifted_count"])):
        assert [y["slot"][d] for d in range(1, degree + 1) if y["kind"][d] == kind] == list(range(held))
    if ps:
        h = ps + 1
        for i in range(1, y["H"] + 1):
            assert (y["kind"][i * h], y["slot"][i * h]) == (2, i - 1)
    if y["use_ps"]:
        assert y["lifted_count"] == y["H"]
        inner = y["H"] - (1 if y["r"] == 0 else 0)                # the evaluation's inner polynomials i = 1 .. (bin_bundle.cpp:225-227,258-264)
        for i in range(0, inner + 1):
            assert (y["kind"][i * h + 1], y["slot"][i * h + 1]) == (1, i * ps)
    else:
        assert y["lifted_count"] == 0


def test_small_grid(emu):
    for ps in range(0, 9):
        for degree in range(0, 3 * (ps + 1) + 3):
            for first in (0, 1, 2, 3):
                check(emu, ps, degree, first)


def test_ps_low_degree_one(emu):
    for first in (0, 1, 2, 3):
        for degree in (0, 1):
            assert layout(emu, 1, degree, first) is not None
        for degree in (2, 3, 7):
            assert layout(emu, 1, degree, first) is None            # (layout() holds the message to the existing text)


@pytest.mark.parametrize("name", ALL_PARAM_FILES)
def test_parameter_files(emu, name):
    js = common.param_json(name)
    p = ref.load_params(js)
    first = ref.RefContext.from_params(p).first
    info = np.zeros(64, dtype=np.uint64)
    assert emu.emu_params_info(js.encode(), info.ctypes.data_as(u64p), 64) > 0
    assert int(info[2]) == first
    for degree in (p["max_items_per_bin"], p["max_items_per_bin"] - 1):
        check(emu, p["ps_low_degree"], degree, first)


def test_all_parameter_files_are_covered():
    assert len(ALL_PARAM_FILES) == 36
