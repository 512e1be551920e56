"""CPU tier of the database side's grouping on the device (apsu_amd/csrc/bucket_plan.h) through the emulation of its launches
(apsu_amd/csrc/emu_bulk/bucket.cpp in libapsu_he_hostemu_bulk.so): (i) the digit plan, (ii) the tile geometry, (iii) the wave-rank lane body
against a count over the lanes, (iv) the emulated passes -- every launch as loops over its tiles, waves and lanes -- word for word
against the existing emu_bucket_items (cuckoo_bucket) on the steered cases of tests/bucket_cases.py, (v) the refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bucket_cases
import emu_lib
from emu_lib import vp

BULK_SO = os.path.join(emu_lib.ROOT, "apsu_amd", "libapsu_he_hostemu_bulk.so")
POISON = bucket_cases.POISON


@pytest.fixture(scope="module")
def emu():
    r = subprocess.run(["make", "-C", emu_lib.SRC, "-s", "../libapsu_he_hostemu_bulk.so"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lib = C.CDLL(BULK_SO)
    lib.emu_bulk_last_error.restype = C.c_char_p
    for name in ("emu_bucket_digit_plan", "emu_bucket_geometry", "emu_bucket_wave_rank", "emu_bucket_sort"):
        assert getattr(lib, name).restype is C.c_int                      # (all four return int)
    return lib


# ------------------------------------------------------------------------------------------------------------- the digit plan
@pytest.mark.parametrize("T", [1, 2, 3, 255, 256, 257, 409, 6552, 16384, 65535, 65536, 65537, 2**32 - 1])
def test_digit_plan_covers_the_bits_of_a_location(emu, T):
    out = np.zeros(10, dtype=np.uint32)
    assert emu.emu_bucket_digit_plan(C.c_uint32(T), vp(out)) == 0
    bits, passes, width, shift = int(out[0]), int(out[1]), out[2:6].tolist(), out[6:10].tolist()
    ceil_log2 = (T - 1).bit_length()
    assert bits == ceil_log2 and (1 << bits) >= T and (bits == 0 or (1 << (bits - 1)) < T)
    assert passes == -(-bits // 8)
    assert all(1 <= w <= 8 for w in width[:passes]) and width[passes:] == [0] * (4 - passes)      # no pass is empty, no digit over 8 bits
    assert sum(width[:passes]) == bits                                                              # the passes cover the bits ...
    assert shift[:passes] == [32 + sum(width[:p]) for p in range(passes)]                           # ... without a gap, from the key's bit 32 up
    assert (bits, width[:passes]) == bucket_cases.digit_plan(T)


def test_shipped_parameter_files_take_two_passes(emu):
    import cuckoo_model
    sizes = sorted({T for _, T, _ in cuckoo_model.shipped_pairs()})
    assert sizes[0] >= 257 and sizes[-1] <= 65536
    for T in sizes:
        out = np.zeros(10, dtype=np.uint32)
        emu.emu_bucket_digit_plan(C.c_uint32(T), vp(out))
        assert out[1] == 2, T


# ------------------------------------------------------------------------------------------------------------- the tile geometry
@pytest.mark.parametrize("tile", [256, 512, 8192])
def test_tile_geometry_at_the_edges(emu, tile):
    run = tile // 4
    for entries in (0, 1, tile - 1, tile, tile + 1, 3 * tile + 1, 2**35):
        out = np.zeros(12, dtype=np.uint64)
        assert emu.emu_bucket_geometry(C.c_uint64(entries), C.c_uint32(tile), vp(out)) == 4
        tiles, last = int(out[0]), int(out[1])
        assert tiles == -(-entries // tile)
        assert last == (0 if not entries else entries - (tiles - 1) * tile) and (last >= 1 or not entries) and last <= tile
        assert (int(out[2]), int(out[3])) == (bucket_cases.TILE_MIN, bucket_cases.TILE_STEP)
        runs = out[4:].reshape(4, 2).tolist()
        # the waves' runs are contiguous, in wave order, of tile / 4 keys until the tile ends, and cover the last tile exactly
        assert runs[0][0] == 0 and runs[3][1] == last
        for w in range(4):
            assert runs[w] == [min(w * run, last), min(w * run + run, last)]
            assert (runs[w][1] - runs[w][0]) <= run and (w == 0 or runs[w][0] == runs[w - 1][1])


@pytest.mark.parametrize("tile", [0, 1, 255, 257, 300, 2**20 + 256])
def test_tile_sizes_outside_the_rule_are_refused(emu, tile):
    out = np.zeros(12, dtype=np.uint64)
    assert emu.emu_bucket_geometry(C.c_uint64(1000), C.c_uint32(tile), vp(out)) == -1
    assert b"tile_entries" in emu.emu_bulk_last_error()
    assert emu.emu_bucket_geometry(C.c_uint64(1000), C.c_uint32(2**20), vp(out)) == 4


# ------------------------------------------------------------------------------------------------------------- the lane body
@pytest.mark.parametrize("width", [0, 1, 5, 8])
def test_wave_rank_counts_the_equal_digits_in_lower_lanes(emu, width):
    rng = np.random.default_rng(width)
    full = (1 << 64) - 1
    for valid in (full, 1, 1 << 63, (1 << 37) - 1, int(rng.integers(0, 1 << 63)) | 1 << 63, 0):
        for spread in (1, 3, 1 << width):
            digit = rng.integers(0, min(spread, 1 << width), 64).astype(np.uint32)
            rank, peers = np.full(64, POISON, dtype=np.uint32), np.full(64, POISON, dtype=np.uint32)
            assert emu.emu_bucket_wave_rank(vp(digit), C.c_uint64(valid), C.c_uint32(width), vp(rank), vp(peers)) == 0
            for lane in range(64):
                if not (valid >> lane) & 1:
                    continue                                               # (a lane without a key takes no part and its result is not used)
                same = [l for l in range(64) if (valid >> l) & 1 and digit[l] == digit[lane]]
                assert rank[lane] == sum(1 for l in same if l < lane) and peers[lane] == len(same), (valid, lane)
    assert emu.emu_bucket_wave_rank(vp(np.zeros(64, dtype=np.uint32)), C.c_uint64(full), C.c_uint32(9), vp(rank), vp(peers)) == -1


# ------------------------------------------------------------------------------------------------------------- the passes
def run_sort(emu, locs, T, tile):
    locs = np.ascontiguousarray(locs, dtype=np.uint32)
    count, H = locs.shape
    offsets = np.full(T + 1, POISON, dtype=np.uint64)
    order = np.full(count * H + 1, POISON, dtype=np.uint32)
    total = C.c_uint64(POISON)
    rc = emu.emu_bucket_sort(vp(locs), C.c_uint64(count), C.c_uint32(H), C.c_uint32(T), C.c_uint32(tile), vp(offsets), vp(order), C.byref(total))
    return rc, offsets, order, total.value


@pytest.mark.parametrize("tile", [bucket_cases.TILE_MIN, 0])
def test_emulated_passes_equal_cuckoo_bucket(emu, tile):
    cases = [c for c in bucket_cases.all_cases() if c[3] == tile]
    assert len(cases) > 100
    for name, locs, T, _ in cases:
        want_off, want_order = bucket_cases.reference(locs, T, name)
        rc, offsets, order, total = run_sort(emu, locs, T, tile)
        assert rc == (len(bucket_cases.digit_plan(T)[1]) if len(locs) else 0), (name, emu.emu_bulk_last_error())     # (no item: nothing runs)
        assert total == len(want_order) and (offsets == want_off).all(), name
        assert (order[:total] == want_order).all(), name
        assert (order[total:] == POISON).all(), name                       # nothing behind the total is written


def test_one_bucket_keeps_the_input_order(emu):
    """stability across lanes, waves and tiles, stated without a reference: every entry in one bucket -> order = 0 .. count - 1"""
    for T, loc in ((1, 0), (65537, 65536), (6552, 4000)):
        for count in (1, 255, 256, 257, 1025):
            rc, offsets, order, total = run_sort(emu, np.full((count, 1), loc, dtype=np.uint32), T, 256)
            assert rc >= 0 and total == count and (order[:count] == np.arange(count)).all()
            assert (offsets[:loc + 1] == 0).all() and (offsets[loc + 1:] == count).all()


def test_refusals_write_nothing(emu):
    locs = np.array([[0, 1, 2], [2, 3, 1]], dtype=np.uint32)
    for T, tile, H_locs, text in ((3, 0, locs, b"location 4 is outside"), (0, 0, locs, b"T >= 1"), (4, 100, locs, b"tile_entries"),
                                  (4, 0, np.zeros((2, 9), dtype=np.uint32), b"H <= 8")):
        rc, offsets, order, total = run_sort(emu, H_locs, T, tile)
        assert rc == -1 and text in emu.emu_bulk_last_error(), emu.emu_bulk_last_error()
        assert (offsets == POISON).all() and (order == POISON).all() and total == POISON
    rc, offsets, order, total = run_sort(emu, locs, 4, 0)
    assert rc == 1 and total == 6 and offsets.tolist() == [0, 1, 3, 5, 6] and order[:6].tolist() == [0, 0, 1, 0, 1, 1]
