"""GPU tier: every grouping kernel alone (apsu_amd/csrc/kernels_bucket.hip) through the steps BUCKET_COUNT .. ENTRIES_GATHER of
apsu_he_debug_run_step, which call the launchers that the whole sort calls (apsu_amd/csrc/launch_bucket.h), on the toy context.  The
cases, the models and the checks are those of tests/bucket_step_model.py, which the CPU tier runs through the emulation
(tests/test_bucket_step_model_cpu.py).  Every comparison is exact.  The scan lengths above 8192 words run the kernel's second and later
steps: the carry, the tail of a later step, and the double-buffered vote wtot[step & 1], a race that only this run can show."""
import numpy as np
import pytest

import apsu_amd
import bucket_step_model as M
import common

pytestmark = pytest.mark.gpu

STORE = apsu_amd.engine.STEP_STORE


class Steps:
    """the runner of tests/bucket_step_model.py over the steps: in/out arrays are copies, so a case's inputs stay as they are"""

    def __init__(self, G):
        self.G = G

    def count(self, locs, tile, tile_cnt):
        out = tile_cnt.copy()
        self.G.debug_run_step("bucket_count", 0, [M.u64(locs)], [out], polys=locs.shape[1], terms=tile)
        return out

    def keys(self, locs, tile, tile_base, keys):
        out = keys.copy()
        self.G.debug_run_step("bucket_keys", 0, [M.u64(locs), M.u64(tile_base)], [out], polys=locs.shape[1], terms=tile)
        return out

    def scan(self, vals, out, total):
        out = out.copy()
        total = None if total is None else total.copy()
        self.G.debug_run_step("bucket_scan", 0, [M.u64(vals) if len(vals) else None], [out, total], flags=STORE if total is not None else 0)
        return out, total

    def hist(self, keys, total, tile, batch, shift, width, hist, wave_cnt):
        h, w = hist.copy(), wave_cnt.copy()
        self.G.debug_run_step("bucket_hist", 0, [M.u64(keys), M.u64([total])], [h, w], terms=tile, batch=batch, e0=shift, n_ext=width)
        return h, w

    def scatter(self, keys, total, tile, batch, shift, width, scanned, wave_cnt, out):
        out = out.copy()
        self.G.debug_run_step("bucket_scatter", 0, [M.u64(keys), M.u64([total]), M.u64(scanned), M.u64(wave_cnt)], [out], terms=tile, batch=batch,
                              e0=shift, n_ext=width)
        return out

    def offsets(self, keys, total, T, out):
        out = out.copy()
        self.G.debug_run_step("bucket_offsets", 0, [M.u64(keys) if len(keys) else None, M.u64([total])], [out], terms=T)
        return out

    def order(self, keys, total, out):
        out = out.copy()
        self.G.debug_run_step("bucket_order", 0, [M.u64(keys) if len(keys) else None, M.u64([total])], [out])
        return out

    def gather(self, items, order, total, out):
        out = np.ascontiguousarray(out.copy())
        self.G.debug_run_step("entries_gather", 0, [M.u64(items), M.u64(order), M.u64([total])], [out], batch=len(order))
        return out


@pytest.fixture(scope="module")
def run():
    G = apsu_amd.HeContext(common.toy_json())
    yield Steps(G)
    G.close()


def test_scan_steps_lanes_waves_and_carry(run):
    """n in {0, 1, 7, 8, 9, 511, 512, 513, 8191, 8192, 8193, 16384, 3 * 8192 + 5, 100003} x {zeros, ones, all 0xFFFFFFFF, random}, with
    and without the sum pointer"""
    assert M.check_scan(run) == len(M.SCAN_LENGTHS) * 4 * 2


def test_histogram_per_tile_and_wave(run):
    """tiles of 256, 512 and 8192 keys; grids of 1, 3 and 40 tiles; totals around a round, a wave's run and a tile, and totals that leave
    the last two tiles empty; widths 1 .. 8 at shifts 32, 40, 56 and 63; keys that show masking, 64 peers a round, the end digits"""
    assert M.check_hist(run) == len(M.hist_cases())


def test_scatter_with_true_gapped_and_inflated_arrays(run):
    """the same cases, each with the true scanned and wave_cnt, with 3 free words in front of every (digit, tile) cell over poison, and
    with wave 0's counts one too large"""
    assert M.check_scatter(run) == 3 * len(M.hist_cases())


def test_count_and_keys_over_the_callers_bases(run):
    """H in {1, 3, 8}, every collision pattern inside an item, counts around 256 and around the tile, 5 free words in front of every tile"""
    assert M.check_count_and_keys(run) == len(M.key_cases())


def test_offsets_and_order_below_the_total(run):
    assert M.check_offsets_and_order(run) == len(M.sorted_key_cases())


def test_gather_below_the_total(run):
    assert M.check_gather(run) == len(M.gather_cases())


def test_refusals_launch_nothing_and_write_nothing(run):
    G = run.G
    P, P32 = M.POISON, M.POISON32
    keys, one = np.zeros(256, dtype=np.uint64), M.u64([1])

    def refused(match, step, ins, outs, **kw):
        before = [o.copy() for o in outs if o is not None]
        with pytest.raises(ValueError, match=match):
            G.debug_run_step(step, 0, ins, outs, **kw)
        assert all((o == b).all() for o, b in zip([o for o in outs if o is not None], before))

    hist = lambda width: [M.poisoned(1 << width, P32), M.poisoned(4 << width, P32)]
    for tile in (0, 255, 257, 300, (1 << 20) + 256):
        refused("tile size", "bucket_hist", [keys, one], hist(1), terms=tile, batch=1, e0=32, n_ext=1)
        refused("tile size", "bucket_count", [keys], [M.poisoned(1, P32)], terms=tile, polys=1)
    for width in (0, 9):
        refused("width", "bucket_hist", [keys, one], hist(1), terms=256, batch=1, e0=32, n_ext=width)
    refused("shift", "bucket_hist", [keys, one], hist(1), terms=256, batch=1, e0=31, n_ext=1)
    refused("shift", "bucket_hist", [keys, one], hist(8), terms=256, batch=1, e0=57, n_ext=8)
    refused("total above", "bucket_hist", [keys, M.u64([257])], hist(1), terms=256, batch=1, e0=32, n_ext=1)
    refused("wrong size", "bucket_hist", [keys, one], hist(2), terms=256, batch=1, e0=32, n_ext=1)
    refused("wrong size", "bucket_hist", [keys[:255], one], hist(1), terms=256, batch=1, e0=32, n_ext=1)
    for H in (0, 9):
        refused("H ", "bucket_count", [np.zeros(18, dtype=np.uint64)], [M.poisoned(1, P32)], terms=256, polys=H)
    refused("32 bits", "bucket_count", [M.u64([1 << 32])], [M.poisoned(1, P32)], terms=256, polys=1)
    refused("wrong size", "bucket_count", [keys], [M.poisoned(2, P32)], terms=256, polys=1)
    # keys: tile 0's three keys from place 2 on in a room of 4
    refused("beyond the room", "bucket_keys", [np.zeros(3, dtype=np.uint64), M.u64([2])], [M.poisoned(4)], terms=256, polys=1)
    # scatter: wave 0's 64 keys of digit 0 from place 3 on in a room of 66; a wave_cnt that moves wave 1's one key beyond a room of 68
    scanned, wc = M.u64([3, 0]), np.zeros(8, dtype=np.uint64)
    refused("beyond the room", "bucket_scatter", [keys, M.u64([65]), scanned, wc], [M.poisoned(66)], terms=256, batch=1, e0=32, n_ext=1)
    wc[0] = 64
    out = M.poisoned(68)
    G.debug_run_step("bucket_scatter", 0, [keys, M.u64([65]), scanned, wc], [out], terms=256, batch=1, e0=32, n_ext=1)
    assert (out[:3] == P).all() and (out[3:68] == 0).all()
    wc[0] = 65
    refused("beyond the room", "bucket_scatter", [keys, M.u64([65]), scanned, wc], [M.poisoned(68)], terms=256, batch=1, e0=32, n_ext=1)
    refused("without STORE", "bucket_scan", [one], [M.poisoned(2), M.poisoned(1)])
    refused("wrong size", "bucket_scan", [one], [M.poisoned(1), None])
    refused("T ", "bucket_offsets", [keys, one], [M.poisoned(2)], terms=0)
    refused("total above", "bucket_offsets", [keys[:3], M.u64([4])], [M.poisoned(3)], terms=1)
    refused("do not ascend", "bucket_offsets", [M.u64([5, 4]), M.u64([2])], [M.poisoned(3)], terms=1)
    refused("wrong size", "bucket_order", [keys[:3], M.u64([3])], [M.poisoned(2, P32)])
    refused("names no item", "entries_gather", [np.zeros((5, 2), dtype=np.uint64), M.u64([0, 5]), M.u64([2])], [M.poisoned(4)], batch=2)
    refused("total above", "entries_gather", [np.zeros((5, 2), dtype=np.uint64), M.u64([0, 1]), M.u64([3])], [M.poisoned(4)], batch=2)
    assert M.check_scan(run, lengths=[9]) == 8                                     # the context goes on working
