"""The database side's grouping by location (apsu_amd/csrc/bucket_plan.h): a numpy restatement of the contract and the steered location
cases that the CPU tier (test_bucket_plan_cpu.py) and the GPU (test_gpu_bucket.py) both run.  The reference of every case is the
existing emu_bucket_items (cuckoo_bucket through libapsu_he_hostemu.so); model() is held to it as well.
A case: (name, locs uint32 [count][H], T).  The locations are GIVEN, not hashed: no item set steers digits, tiles and collisions."""
import ctypes as C

import numpy as np

import emu_lib
from emu_lib import vp

TILE_MIN, TILE_STEP, TILE_DEFAULT = 256, 256, 8192      # bucket_plan.h: BUCKET_TILE_MIN, BUCKET_TILE_STEP, BUCKET_TILE_DEFAULT
TABLE_SIZES = [1, 2, 255, 256, 257, 65537]              # one digit, the edges of one and two digits, a third pass
POISON = 0xDEADBEEF


def model(locs, T):
    """the surviving pairs (loc, i) -- entry (i, h) survives unless an earlier function of item i gave the same location -- in ascending
    (loc, i) order -> (offsets [T + 1] uint64, order uint32)"""
    locs = np.asarray(locs, dtype=np.uint32)
    first = np.stack([~(locs[:, :h] == locs[:, h:h + 1]).any(axis=1) for h in range(locs.shape[1])], axis=1)
    loc, i = locs[first], np.nonzero(first)[0]
    keep = np.lexsort((i, loc))
    offsets = np.concatenate([[0], np.cumsum(np.bincount(loc, minlength=T))]).astype(np.uint64)
    return offsets, i[keep].astype(np.uint32)


_EMU = None
_REFERENCE = {}


def reference(locs, T, name=None):
    """emu_bucket_items -> (offsets, order [total]); a named case's is computed once"""
    if name is not None:
        key = (name, T, locs.shape)
        if key not in _REFERENCE:
            _REFERENCE[key] = reference(locs, T)
        return _REFERENCE[key]
    global _EMU
    if _EMU is None:
        _EMU = emu_lib.load()
    locs = np.ascontiguousarray(locs, dtype=np.uint32)
    count, H = locs.shape
    offsets = np.zeros(T + 1, dtype=np.uint64)
    order = np.zeros(max(count * H, 1), dtype=np.uint32)
    total = C.c_uint64()
    assert _EMU.emu_bucket_items(vp(locs), C.c_uint64(count), C.c_uint32(H), C.c_uint32(T), vp(offsets), vp(order), C.byref(total)) == 0
    assert total.value == int(offsets[-1])
    want_off, want_order = model(locs, T)
    assert (offsets == want_off).all() and (order[:total.value] == want_order).all()
    return offsets, order[:total.value].copy()


def digit_plan(T):
    """bucket_digit_plan restated: ceil(log2 T) bits in ceil(bits / 8) digits, as even as whole bits allow, the wider ones first"""
    bits = (T - 1).bit_length()
    passes = -(-bits // 8)
    return bits, [bits // passes + (1 if p < bits % passes else 0) for p in range(passes)]


def _locs(rows, H):
    return np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, H)


def small_cases():
    """count in {0, 1, 63, 64, 65} x H in {1, 3, 8} x every table size: random locations (collisions inside an item come by themselves at
    T = 1 and 2)"""
    out = []
    for T in TABLE_SIZES:
        for H in (1, 3, 8):
            rng = np.random.default_rng(1000 * H + T)
            for count in (0, 1, 63, 64, 65):
                out.append(("%d items, H = %d, T = %d" % (count, H, T), _locs(rng.integers(0, T, (count, H)), H), T))
    return out


def tile_cases(tile):
    """entry counts of tile - 1, tile, tile + 1 and 3 tiles + 1 (H = 1: one entry per item): random, all in one bucket, all in the last
    bucket, two buckets that differ in the high digit alone; function collisions across a tile boundary"""
    out = []
    for entries in (tile - 1, tile, tile + 1, 3 * tile + 1):
        for T in (257, 65537):
            rng = np.random.default_rng(entries + T)
            out.append(("%d random entries, T = %d" % (entries, T), _locs(rng.integers(0, T, (entries, 1)), 1), T))
    n = 3 * tile + 1
    for T in (1, 6552, 65537):
        out.append(("every entry in bucket 0 of %d" % T, np.zeros((n, 1), dtype=np.uint32), T))
        out.append(("every entry in the last bucket of %d" % T, np.full((n, 1), T - 1, dtype=np.uint32), T))
        if T > 1:
            out.append(("every entry in a middle bucket of %d" % T, np.full((n, 1), T // 3, dtype=np.uint32), T))
    for T in (6552, 65537):
        _, widths = digit_plan(T)
        low = sum(widths[:-1])
        a, b = 5, 5 + (1 << low)                          # equal in every digit but the last
        assert b < T and len(widths) >= 2
        out.append(("alternating buckets %d and %d of %d" % (a, b, T), _locs(np.where(np.arange(n) % 2, a, b), 1), T))
        out.append(("runs of 70 in buckets %d and %d of %d" % (b, a, T), _locs(np.where((np.arange(n) // 70) % 2, a, b), 1), T))
    # H = 3, items by turns: distinct, h0 = h1, h0 = h2, h1 = h2, all equal: the entry count falls below 3 count and the keys' tiles (of
    # `tile` items) end where the running count is no multiple of anything
    count = 2 * tile + 3
    rng = np.random.default_rng(tile)
    for T in (257, 6552):
        l = rng.integers(0, T - 3, (count, 3)).astype(np.uint32)
        l[:, 1] = l[:, 0] + 1
        l[:, 2] = l[:, 0] + 2
        kind = np.arange(count) % 5
        l[kind == 1, 1] = l[kind == 1, 0]
        l[kind == 2, 2] = l[kind == 2, 0]
        l[kind == 3, 2] = l[kind == 3, 1]
        l[kind == 4, 1] = l[kind == 4, 0]
        l[kind == 4, 2] = l[kind == 4, 0]
        out.append(("function collisions inside the items, T = %d" % T, l, T))
    out.append(("every function of every item on one location", np.full((count, 3), 7, dtype=np.uint32), 9))
    out.append(("every function of every item on one location, H = 8", np.full((tile + 1, 8), 1, dtype=np.uint32), 2))
    return out


def random_cases():
    out = []
    for T in (409, 6552):
        out.append(("5000 random items in %d slots" % T, _locs(np.random.default_rng(T).integers(0, T, (5000, 3)), 3), T))
    return out


def all_cases():
    """(name, locs, T, tile): every case at the least tile and at the default"""
    out = []
    for name, locs, T in small_cases() + random_cases():
        out += [(name, locs, T, TILE_MIN), (name, locs, T, 0)]
    for tile in (TILE_MIN, TILE_DEFAULT):
        out += [(name, locs, T, tile if tile == TILE_MIN else 0) for name, locs, T in tile_cases(tile)]
    return out
