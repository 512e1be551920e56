"""The one way to the CPU emulation library (apsu_amd/libapsu_he_hostemu.so; sources: apsu_amd/csrc/emu/).

load() asks make for the library every time, once per process: the Makefile knows from the compiler's own dependency files
(build/*.d) when an object is older than a header it read, so a test never runs against code that is no longer in the tree, and on a
current tree the call costs a few milliseconds.  The table below declares the return type of every export that does not return int;
ctypes would otherwise cut a 64-bit result to 32 bits without a word (tests/test_emu_lib_cpu.py holds the table to the sources)."""
import ctypes as C
import functools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "apsu_amd", "csrc")
SO = os.path.join(ROOT, "apsu_amd", "libapsu_he_hostemu.so")

RESTYPES = {
    "emu_last_error": C.c_char_p,
    "emu_packed_coeff": C.c_uint64, "emu_field_generator": C.c_uint64, "emu_bin_unlift": C.c_uint64, "emu_qs_block": C.c_uint64,
    "emu_bin_roots": C.c_int64, "emu_bins_rows": C.c_int64, "emu_rebase_plan": C.c_int64, "emu_split_parts": C.c_int64,
    "emu_device_constants": C.c_int64, "emu_roots_coset_count": C.c_int64, "emu_bin_update": C.c_int64,
    "emu_split_cut": C.c_uint32, "emu_split_part_of": C.c_uint32, "emu_split_capacity": C.c_uint32, "emu_merge_fold_interval": C.c_uint32,
    "emu_packed_row_bits": C.c_uint32,
    "emu_ntt_form": None, "emu_dev_layout": None, "emu_switches": None, "emu_bin_counts": None, "emu_self_test_reduce": None,
    "emu_packed_pair": None, "emu_mac_rules": None, "emu_cuckoo_tables": None, "emu_query_values": None,
}


@functools.lru_cache(maxsize=None)
def make_current():
    """ask make for the library, once per process; a failed make raises with the compiler's output"""
    r = subprocess.run(["make", "-C", SRC, "-s", "../libapsu_he_hostemu.so"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        raise RuntimeError("make ../libapsu_he_hostemu.so failed (exit %d):\n%s" % (r.returncode, r.stdout))


def load():
    """the library, made current first.  Every call returns a handle of its own to the one loaded library, so that the `argtypes` a test
    module declares for its own calls (pointer types differ between modules) stay with that module."""
    make_current()
    lib = C.CDLL(SO)
    for name, restype in RESTYPES.items():
        getattr(lib, name).restype = restype
    return lib


def vp(a):
    """a numpy array's buffer as a pointer argument"""
    return C.c_void_p(a.ctypes.data)
