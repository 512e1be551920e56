"""CPU tier: the build's dependencies are the ones the compiler wrote down (apsu_amd/csrc/Makefile, build/*.d), unit by unit.

The device code is split by kernel family so that work on anything but the transforms does not pay for the transforms' object
(kernels_ntt.o: minutes; every other unit: seconds).  That holds only while no header of another family is reachable from
kernels_ntt.hip, and while every object that does read a header is remade with it.  Asked of make itself, on the built tree:
`make -n -W <header> all` lists what an edit of that header would compile."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "apsu_amd", "csrc")
EMU = "../libapsu_he_hostemu.so"


def remade(header):
    """the targets (objects under build/, libraries) whose commands make would run after an edit of `header`"""
    dep = os.path.join(SRC, "build", "kernels_ntt.d")
    assert os.path.exists(dep), ("%s is missing: build the tree first (python __graft_entry__.py, or make -C apsu_amd/csrc all), "
                                 "the compile step writes the dependency files" % dep)
    assert os.path.exists(os.path.join(SRC, header))
    out = subprocess.run(["make", "-C", SRC, "-n", "-W", header, "all"], check=True, capture_output=True, text=True).stdout
    return set(re.findall(r" -o (\S+)", out))


@pytest.mark.parametrize("header, unit", [("bin_merge.h", "kernels_db.o"), ("bin_update.h", "kernels_db.o"),
                                          ("mac_core.h", "kernels_mac.o"), ("query_side.h", "kernels_ew.o"),
                                          ("query_side.h", "engine_query_steps.o"), ("query_side.h", "emu/query.o"),
                                          ("mac_core.h", "engine_mac_steps.o"), ("mac_plan.h", "engine_mac_steps.o"),
                                          ("mac_plan.h", "kernels_mac.o"), ("mac_plan.h", "emu/mac.o")])
def test_family_header_spares_the_transforms(header, unit):
    got = remade(header)
    assert "build/" + unit in got, got
    assert "build/kernels_ntt.o" not in got, got


@pytest.mark.parametrize("header, units", [("cuckoo.h", {"build/emu/cuckoo.o", "build/kernels_cuckoo.o"}), ("mac_core.h", {"build/emu/mac.o"})])
def test_family_header_spares_the_transform_emulation(header, units):
    """the emulation library is in units by family too (apsu_amd/csrc/emu/): the transforms' unit is its long one"""
    got = remade(header)
    assert units | {EMU} <= got, got
    assert "build/emu/ntt.o" not in got and "build/kernels_ntt.o" not in got, got


def kernel_objects(got):
    return {t for t in got if t.startswith("build/kernels_")}


def test_evaluation_plan_spares_the_other_engine_units():
    """the Engine is in units by section (engine_impl.h): the evaluation's plan is read by the evaluation, not by ComputePowers, the
    querier's side or the paths without key switching"""
    got = remade("eval_plan.h")
    assert {"build/engine_eval.o", "build/kernels_behz.o", "build/emu/rules.o"} <= got, got
    assert not {"build/engine_powers.o", "build/engine_query.o", "build/engine_query_steps.o", "build/engine_nks.o"} & got, got
    assert "build/kernels_ntt.o" not in got, got


def test_powers_schedule_reaches_its_users_and_no_kernel():
    got = remade("powers_sched.h")
    assert {"build/engine.o", "build/engine_powers.o", "build/engine_nks.o", "build/emu/rules.o", EMU} <= got, got
    assert not kernel_objects(got), got


def test_transform_header_reaches_every_user():
    got = remade("ntt_core.h")
    assert {"build/kernels_ntt.o", "build/kernels_roots.o", EMU} <= got, got
