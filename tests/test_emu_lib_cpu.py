"""CPU tier: the loader of the CPU emulation library (tests/emu_lib.py) against the library's sources (apsu_amd/csrc/emu/*.cpp).

ctypes takes every foreign function to return int unless told otherwise and cuts a wider result to 32 bits without a word, so the
loader's table of return types has to name exactly the exports that do not return int; and what the sources define has to be what
the library exports, so that a unit left out of the build (or a stale library) shows here and not as a missing attribute somewhere."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np

import emu_lib
from emu_lib import vp
from test_bundle_merge_cpu import T60

CTYPE = {"const char *": C.c_char_p, "uint64_t": C.c_uint64, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "void": None}
# a definition at the left margin inside an extern "C" block: return type, name, parameters, then the body (a declaration ends in ';')
DEFINITION = re.compile(r"^((?:const )?\w+ \*?)(emu_\w+)\([^;{]*?\)\s*\{", re.M)


def defined_in_sources():
    """name -> declared return type of every extern "C" definition named emu_*"""
    found = {}
    for path in sorted(glob.glob(os.path.join(emu_lib.SRC, "emu", "*.cpp"))):
        for block in re.findall(r'^extern "C" \{$(.*?)^\} // extern "C"$', open(path).read(), re.M | re.S):
            for ret, name in DEFINITION.findall(block):
                assert name not in found, name + " is defined twice"
                found[name] = ret.strip()
    return found


def test_return_types_cover_every_export():
    lib = emu_lib.load()
    src = defined_in_sources()
    out = subprocess.run(["nm", "-D", "--defined-only", emu_lib.SO], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (emu_\w+)$", out, re.M))
    assert set(src) == exported and len(exported) == 87, sorted(set(src) ^ exported)
    assert all(ret == "int" or ret in CTYPE for ret in src.values()), sorted(set(src.values()))
    assert {n: CTYPE[ret] for n, ret in src.items() if ret != "int"} == emu_lib.RESTYPES
    for name, restype in emu_lib.RESTYPES.items():
        assert getattr(lib, name).restype is restype, name


def test_results_wider_than_32_bits_arrive_whole():
    """three uint64_t exports whose true results do not fit 32 bits, through load() alone"""
    lib = emu_lib.load()
    # a row of 64-bit coefficients as 32-bit words (mac_core.h packed_coeff): coefficient 1
    coeffs = [0x0123456789ABCDEF, 0xFEDCBA9876543210, 0x8000000000000001]
    row = np.array([w for c in coeffs for w in (c & 0xFFFFFFFF, c >> 32)] + [0, 0], dtype=np.uint32)
    for i, c in enumerate(coeffs):
        assert lib.emu_packed_coeff(vp(row), C.c_uint64(i), C.c_uint32(64)) == c
    # a stored coefficient of a 60-bit plain modulus under a 61-bit first prime (bin_update.h bin_unlift): below t as it is, above it shifted
    q0 = (1 << 61) - 1
    for x in (T60 - 1, q0 - 1, q0 - (T60 - 1) // 2):
        want = x if x < T60 else x - (q0 - T60)
        assert want >> 32 and lib.emu_bin_unlift(C.c_uint64(x), C.c_uint64(T60), C.c_uint64(q0)) == want
    # the stream block of the last object's last noise coefficient (query_side.h qs_noise_block): beyond 2^32
    lay = np.zeros(7, dtype=np.uint64)
    assert lib.emu_qs_layout(vp(lay), 7) == 7
    max_n, poly_blocks, _, max_objects, _, _, noise0 = (int(v) for v in lay)
    obj, k = max_objects - 1, max_n - 1
    want = noise0 + obj * poly_blocks + k // 8
    assert want > 1 << 32 and lib.emu_qs_block(2, C.c_uint64(obj), C.c_uint64(k)) == want
