"""CPU tier: every grouping kernel alone (apsu_amd/csrc/kernels_bucket.hip) through the per-kernel entry points of its emulation
(apsu_amd/csrc/emu_bulk/bucket.cpp in libapsu_he_hostemu_bulk.so), held to the models of tests/bucket_step_model.py on the cases the GPU
tier runs through the steps (tests/test_gpu_bucket_steps.py).  The scan's emulation steps as the kernel does -- 8192 words a step, eight
words a lane, the waves' inclusive sums, the carry -- so the multi-step lengths mean here what they mean on the device; what a serial
emulation cannot show is the double-buffered vote (wtot[step & 1]): a race, guarded by the GPU run of those lengths alone.  The models
are held to emu_bucket_items (cuckoo_bucket) on the pipeline cases of tests/bucket_cases.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bucket_cases
import bucket_step_model as M
import emu_lib
from emu_lib import vp

BULK_SO = os.path.join(emu_lib.ROOT, "apsu_amd", "libapsu_he_hostemu_bulk.so")
u64, u32 = C.c_uint64, C.c_uint32


def narrow(x):
    assert (x >> np.uint64(32) == 0).all()
    return np.ascontiguousarray(x, dtype=np.uint32).reshape(-1)


class Emu:
    """the runner of tests/bucket_step_model.py over the emulation: 32-bit arrays are narrowed on the way in and widened on the way out"""

    def __init__(self, lib):
        self.lib = lib

    def ok(self, rc):
        assert rc == 0, self.lib.emu_bulk_last_error()

    def count(self, locs, tile, tile_cnt):
        l, c = narrow(locs), narrow(tile_cnt)
        self.ok(self.lib.emu_bucket_count(vp(l), u64(locs.shape[0]), u32(locs.shape[1]), u32(tile), vp(c)))
        return c.astype(np.uint64)

    def keys(self, locs, tile, tile_base, keys):
        l, out = narrow(locs), keys.copy()
        self.ok(self.lib.emu_bucket_keys(vp(l), u64(locs.shape[0]), u32(locs.shape[1]), u32(tile), vp(M.u64(tile_base)), vp(out), u64(len(out))))
        return out

    def scan(self, vals, out, total):
        v, out = narrow(vals), out.copy()
        total = None if total is None else total.copy()
        self.ok(self.lib.emu_bucket_scan(vp(v), u64(len(v)), vp(out), vp(total) if total is not None else None))
        return out, total

    def hist(self, keys, total, tile, batch, shift, width, hist, wave_cnt):
        h, w = narrow(hist), narrow(wave_cnt)
        self.ok(self.lib.emu_bucket_hist(vp(M.u64(keys)), u64(total), u64(batch), u32(tile), u32(shift), u32(width), vp(h), vp(w)))
        return h.astype(np.uint64), w.astype(np.uint64)

    def scatter(self, keys, total, tile, batch, shift, width, scanned, wave_cnt, out):
        out, w = out.copy(), narrow(wave_cnt)
        self.ok(self.lib.emu_bucket_scatter(vp(M.u64(keys)), u64(total), u64(batch), u32(tile), u32(shift), u32(width), vp(M.u64(scanned)), vp(w), vp(out),
                                            u64(len(out))))
        return out

    def offsets(self, keys, total, T, out):
        out = out.copy()
        self.ok(self.lib.emu_bucket_offsets(vp(M.u64(keys)), u64(total), u32(T), vp(out)))
        return out

    def order(self, keys, total, out):
        o = narrow(out)
        self.ok(self.lib.emu_bucket_order(vp(M.u64(keys)), u64(total), vp(o)))
        return o.astype(np.uint64)

    def gather(self, items, order, total, out):
        out, o = out.copy(), np.ascontiguousarray(order).astype(np.uint32)
        self.ok(self.lib.emu_entries_gather(vp(M.u64(items)), u64(len(items)), vp(o), u64(total), vp(out)))
        return out


@pytest.fixture(scope="module")
def emu():
    r = subprocess.run(["make", "-C", emu_lib.SRC, "-s", "../libapsu_he_hostemu_bulk.so"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lib = C.CDLL(BULK_SO)
    lib.emu_bulk_last_error.restype = C.c_char_p
    return Emu(lib)


def test_scan_steps_lanes_waves_and_carry(emu):
    assert M.check_scan(emu) == len(M.SCAN_LENGTHS) * 4 * 2
    assert M.SCAN_STEP == 8192 and sum(1 for n in M.SCAN_LENGTHS if n > M.SCAN_STEP) >= 4      # lengths of two, three, four and 13 steps


def test_histogram_per_tile_and_wave(emu):
    assert M.check_hist(emu) == len(M.hist_cases()) >= 130


def test_scatter_with_true_gapped_and_inflated_arrays(emu):
    assert M.check_scatter(emu) == 3 * len(M.hist_cases())


def test_count_and_keys_over_the_callers_bases(emu):
    assert M.check_count_and_keys(emu) == len(M.key_cases()) == 39


def test_offsets_and_order_below_the_total(emu):
    assert M.check_offsets_and_order(emu) > 80


def test_gather_below_the_total(emu):
    assert M.check_gather(emu) == 24


def test_entry_points_refuse_what_the_steps_refuse(emu):
    lib = emu.lib
    keys, out = np.zeros(256, dtype=np.uint64), M.poisoned(4)
    wc, sc = np.zeros(4 * 2, dtype=np.uint32), np.array([3, 0], dtype=np.uint64)
    # 65 keys of digit 0 from place 3 on, in a room of 4 words
    wc[0] = 1
    assert lib.emu_bucket_scatter(vp(keys), u64(65), u64(1), u32(256), u32(32), u32(1), vp(sc), vp(wc), vp(out), u64(4)) == -1
    assert b"beyond the room" in lib.emu_bulk_last_error() and (out == M.POISON).all()
    for tile, shift, width in ((255, 32, 1), (256, 31, 1), (256, 32, 9), (256, 32, 0), (256, 57, 8)):
        h, w = np.zeros(512, dtype=np.uint32), np.zeros(2048, dtype=np.uint32)
        assert lib.emu_bucket_hist(vp(keys), u64(1), u64(1), u32(tile), u32(shift), u32(width), vp(h), vp(w)) == -1
    assert lib.emu_bucket_hist(vp(keys), u64(257), u64(1), u32(256), u32(32), u32(1), vp(h), vp(w)) == -1
    locs = np.zeros(9, dtype=np.uint32)
    assert lib.emu_bucket_count(vp(locs), u64(1), u32(9), u32(256), vp(h)) == -1
    base = np.array([2], dtype=np.uint64)
    assert lib.emu_bucket_keys(vp(locs), u64(3), u32(1), u32(256), vp(base), vp(out), u64(4)) == -1 and (out == M.POISON).all()
    assert lib.emu_bucket_offsets(vp(keys), u64(0), u32(0), vp(out)) == -1
    order = np.array([0, 5], dtype=np.uint32)
    assert lib.emu_entries_gather(vp(keys), u64(5), vp(order), u64(2), vp(out)) == -1 and (out == M.POISON).all()


def test_models_equal_cuckoo_bucket_on_the_pipeline_cases():
    """the models composed as launch_bucket_sort composes the kernels, against emu_bucket_items: every steered case at the least tile"""
    cases = [c for c in bucket_cases.all_cases() if c[3] == bucket_cases.TILE_MIN and len(c[1])]
    assert len(cases) > 90
    for name, locs, T, tile in cases:
        want_off, want_order = bucket_cases.reference(locs, T, name)
        offsets, order = M.pipeline_model(locs, T, tile, bucket_cases.digit_plan(T)[1])
        assert (offsets == want_off).all() and (order == want_order).all(), name
