"""CPU tier of building a whole database from its entries (apsu_amd/csrc/bulk_place.h): (i) the closed form of the placement rule --
bulk_plan through emu_bulk_plan, bulk_chunk through what emu_entries_scatter writes -- held to two references, a Python restatement of
the reference's loop from an empty database (ReceiverDB::insert_or_assign_worker, receiver_db.cpp:349-434) and the existing
emu_place_entries with no BinBundle given; (ii) the lane body of k_entries_scatter, stepped over every lane of its grid by
emu_entries_scatter, held to a Python bit split, with a sentinel in every word nobody may write; (iii) every refusal of bulk_plan.
All comparisons are exact integers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_lib
from emu_lib import vp
from test_bundle_lookup_cpu import run_place

SENTINEL = 0xEEEEEEEEEEEEEEEE
SENT32 = 0xEEEEEEEE


BULK_SO = os.path.join(emu_lib.ROOT, "apsu_amd", "libapsu_he_hostemu_bulk.so")


class Both:
    """the two emulation libraries behind one name: emu_bulk_plan / emu_entries_scatter live in a library of their own
    (apsu_amd/csrc/emu_bulk/), made current by make like the other (emu_lib.make_current); everything else is emu_lib.load()'s"""

    def __init__(self):
        r = subprocess.run(["make", "-C", emu_lib.SRC, "-s", "../libapsu_he_hostemu_bulk.so"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        self.bulk = C.CDLL(BULK_SO)
        self.bulk.emu_bulk_last_error.restype = C.c_char_p
        self.emu_bulk_plan, self.emu_entries_scatter = self.bulk.emu_bulk_plan, self.bulk.emu_entries_scatter    # (both return int)
        self.emu_last_error = self.bulk.emu_bulk_last_error
        self.rest = emu_lib.load()

    def __getattr__(self, name):
        return getattr(self.rest, name)


@pytest.fixture(scope="module")
def emu():
    return Both()


# ------------------------------------------------------------------------------------------------------------- models
def felt(item, j, bpf, item_bits):
    """algebraize_item's bit split: felt j = bits [j bpf, j bpf + bpf) of the item's first item_bits bits (a Python integer)"""
    off = j * bpf
    take = max(0, min(bpf, item_bits - off))
    return (item >> off) & ((1 << take) - 1)


def model_loop(counts, ipb, max_items):
    """The reference's loop from an empty database over locations with `counts` entries each: per bundle index the BinBundles as lists of
    per-location entry lists.  -> (bundles[b][k][loc] = [entry positions i in arrival order], target[l][i] = k)"""
    nb = len(counts) // ipb
    bundles = [[] for _ in range(nb)]
    target = []
    for l, c in enumerate(counts):
        b, loc = divmod(l, ipb)
        tl = []
        for i in range(c):
            k = next((k for k in reversed(range(len(bundles[b]))) if len(bundles[b][k][loc]) + 1 < max_items), None)   # newest first, strictly
            if k is None:
                bundles[b].append([[] for _ in range(ipb)])     # a fresh BinBundle takes the entry unconditionally
                k = len(bundles[b]) - 1
            bundles[b][k][loc].append(i)
            tl.append(k)
        target.append(tl)
    return bundles, target


def plan(emu, counts, ipb, max_items):
    T = len(counts)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    kstart = np.full(max(T, 1), SENT32, dtype=np.uint32)
    per_index = np.full(max(T // ipb, 1), SENT32, dtype=np.uint32)
    total = C.c_uint64(SENTINEL)
    rc = emu.emu_bulk_plan(vp(offsets), C.c_uint64(T), C.c_uint32(ipb), C.c_uint32(max_items), vp(kstart), vp(per_index), C.byref(total))
    assert rc == 0, emu.emu_last_error()
    assert total.value == int(per_index[:T // ipb].sum())
    return offsets, kstart[:T], per_index[:T // ipb]


def scatter(emu, items, offsets, kstart, F, bpf, item_bits, cap, k, stride, bins, n_counts, blocks=0):
    """emu_entries_scatter for one bundle index's slices -> (roots [bins][stride], counts [n_counts]), sentinels where nothing was written"""
    locations = len(kstart)
    words = np.array([[it & (2 ** 64 - 1), it >> 64] for it in items], dtype=np.uint64).reshape(len(items), 2)
    roots = np.full((bins, stride), SENTINEL, dtype=np.uint64)
    cnt = np.full(n_counts, SENT32, dtype=np.uint32)
    rc = emu.emu_entries_scatter(vp(words), vp(np.ascontiguousarray(offsets)), vp(np.ascontiguousarray(kstart)), C.c_uint32(locations), C.c_uint32(F), C.c_uint32(bpf),
                                 C.c_uint32(item_bits), C.c_uint32(cap), C.c_uint32(k), C.c_uint32(stride), C.c_uint32(bins), vp(roots), vp(cnt),
                                 C.c_uint32(n_counts), C.c_uint32(blocks))
    assert rc >= 1, emu.emu_last_error()
    return roots, cnt


def check_shape(emu, rng, counts, ipb, F, max_items, bpf=13):
    """both references against the plan and the scatter's outputs for one vector of per-location counts"""
    cap = max_items - 1
    item_bits = bpf * F
    T, nb = len(counts), len(counts) // ipb
    offsets, kstart, per_index = plan(emu, counts, ipb, max_items)
    bundles, target = model_loop(counts, ipb, max_items)
    assert [len(x) for x in bundles] == [int(v) for v in per_index]
    # K_l: the BinBundles of the index when location l begins
    for l in range(T):
        b, loc = divmod(l, ipb)
        seen = max([0] + [-(-counts[b * ipb + p] // cap) for p in range(loc)])
        assert int(kstart[l]) == seen
    # distinct items per location (the contract's precondition); their felts are then distinct per location too, F * bpf bits each
    total = int(offsets[-1])
    items = [int(v) for v in rng.choice(1 << min(20, item_bits), size=total, replace=False)] if total else []
    items = [(v * 0x9E3779B97F4A7C15F39CC0605CEDC835) % (1 << item_bits) | ((i & 0xFF) << item_bits) for i, v in enumerate(items)]   # (bits above item_bits are ignored)
    bins, n_counts = ipb * F + 2, ipb * F + 5
    for b in range(nb):
        lo = b * ipb
        off_b, ks_b = offsets[lo:lo + ipb + 1], kstart[lo:lo + ipb]
        its = items[int(off_b[0]):int(off_b[-1])]
        # reference two: place_entries from no BinBundle, entries in arrival order
        ins = [((l - lo) * F, [felt(items[int(offsets[l]) + i], j, bpf, item_bits) for j in range(F)]) for l in range(lo, lo + ipb) for i in range(counts[l])]
        placed = None
        if ins:
            rc, placed = run_place(emu.rest, [], ins, [], F, ipb * F, max_items, t=(1 << 61) - 1)
            assert rc == 0, placed
            assert placed["n_new"] == len(bundles[b]) and all(s == 0 for s in placed["ins_status"])
            assert placed["ins_target"] == [k for l in range(lo, lo + ipb) for k in target[l]]
        for k in range(len(bundles[b])):
            degree = max(len(x) for x in bundles[b][k])
            assert degree >= 1
            stride = degree + int(rng.integers(0, 3))
            roots, cnt = scatter(emu, its, off_b, ks_b, F, bpf, item_bits, cap, k, stride, bins, n_counts, blocks=int(rng.integers(0, 3)))
            want = np.full((bins, stride), SENTINEL, dtype=np.uint64)
            for loc in range(ipb):
                here = bundles[b][k][loc]
                for j in range(F):
                    assert int(cnt[loc * F + j]) == len(here)
                    for r, i in enumerate(here):                  # position in the bin = arrival order in that BinBundle
                        want[loc * F + j, r] = felt(items[int(offsets[lo + loc]) + i], j, bpf, item_bits)
                    if placed is not None:                        # the same per-bin lists, in the same order
                        assert placed["ins_lists"][k].get(loc * F + j, []) == [int(v) for v in want[loc * F + j, :len(here)]]
            assert (cnt[ipb * F:] == 0).all()
            assert (roots == want).all()


# ------------------------------------------------------------------------------------------------------------- the rule
def test_closed_form_on_random_shapes(emu):
    rng = np.random.default_rng(0x42554C4B)
    for trial in range(60):
        nb, ipb, F, max_items = int(rng.integers(1, 4)), int(rng.integers(1, 13)), int(rng.integers(1, 6)), int(rng.integers(2, 7))
        cap = max_items - 1
        menu = [0, 1, cap - 1, cap, cap + 1, 2 * cap, 3 * cap + 1, int(rng.integers(0, 4 * cap + 2))]
        counts = [int(menu[int(rng.integers(0, len(menu)))]) for _ in range(nb * ipb)]
        check_shape(emu, rng, counts, ipb, F, max_items)


@pytest.mark.parametrize("name, counts, ipb, max_items", [
    # cap = 4 throughout
    ("an empty location between full ones", [4, 0, 4, 8, 0, 8], 6, 5),
    ("a later location fills the newest BinBundles first", [12, 6, 1, 9], 4, 5),          # K = 3: 6 entries -> BinBundles 2, 1; 1 -> 2; 9 -> 2, 1, 0
    ("a location fills every BinBundle and opens two more", [8, 16, 3], 3, 5),            # K = 2, 16 entries: 1, 0, then 2, 3
    ("K restarts with the second bundle index", [12, 5, 0, 6, 2, 0], 3, 5),               # location 3 begins with no BinBundle
    ("cap = 1: every entry its own BinBundle", [3, 1, 0, 2], 2, 2),
])
def test_closed_form_on_edge_vectors(emu, name, counts, ipb, max_items):
    check_shape(emu, np.random.default_rng(7), counts, ipb, F=3, max_items=max_items)


def test_edge_vector_targets_by_hand(emu):
    """the second edge vector spelled out: which BinBundle every entry of every location goes to"""
    _, target = model_loop([12, 6, 1, 9], 4, 5)
    assert target[0] == [0] * 4 + [1] * 4 + [2] * 4
    assert target[1] == [2] * 4 + [1] * 2                                  # newest first, in reversed order
    assert target[2] == [2]
    assert target[3] == [2] * 4 + [1] * 4 + [0]
    offsets, kstart, per_index = plan(emu, [12, 6, 1, 9], 4, 5)
    assert [int(v) for v in kstart] == [0, 3, 3, 3] and [int(v) for v in per_index] == [3]


# ------------------------------------------------------------------------------------------------------------- the lane body
@pytest.mark.parametrize("bpf, F, item_bits", [
    (16, 5, 80),                                             # felt 4 starts exactly at bit 64
    (20, 5, 100),                                            # felt 3 crosses bit 64
    (16, 5, 75),                                             # the last felt is short: 11 bits
    (20, 5, 90),                                             # felt 4 holds 10 bits
    (20, 5, 128 - 45),                                       # felt 4 holds 3 bits
])
def test_scatter_bit_split(emu, bpf, F, item_bits):
    rng = np.random.default_rng(bpf * 1000 + item_bits)
    ipb, cap = 12, 300                                       # a chunk longer than one workgroup of 256 lanes
    counts = [0, 1, 299, 300, 301, 64, 65, 600, 0, 257, 3, 255]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64) + np.uint64(1000)      # a slice from the middle of the list
    kstart = np.array([0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2], dtype=np.uint32)
    edge = [0, (1 << 128) - 1, 1 << 63, 1 << 64, (1 << 64) - 1, 0xAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA, 0x5555555555555555AAAAAAAAAAAAAAAA]
    items = [int.from_bytes(rng.bytes(16), "little") for _ in range(sum(counts))]
    items[2:2 + len(edge)] = edge
    bins, n_counts = ipb * F + 4, 64
    for k in (0, 1, 2):
        for blocks in (0, 1, 2, 3):
            stride = 300
            roots, cnt = scatter(emu, items, offsets, kstart, F, bpf, item_bits, cap, k, stride, bins, n_counts, blocks)
            want = np.full((bins, stride), SENTINEL, dtype=np.uint64)
            for loc, c in enumerate(counts):
                ks = int(kstart[loc])
                m = ks - 1 - k if k < ks else k
                first = m * cap
                ln = max(0, min(cap, c - first))
                base = int(offsets[loc] - offsets[0]) + first
                for j in range(F):
                    assert int(cnt[loc * F + j]) == ln
                    for r in range(ln):
                        want[loc * F + j, r] = felt(items[base + r], j, bpf, item_bits)
            assert (cnt[ipb * F:] == 0).all()
            assert (roots == want).all()
    # the short felt really is short, and the split puts the item's first item_bits bits back together
    it = (1 << 128) - 1
    assert felt(it, F - 1, bpf, item_bits) == (1 << (item_bits - (F - 1) * bpf)) - 1
    assert sum(felt(it, j, bpf, item_bits) << (j * bpf) for j in range(F)) == (1 << item_bits) - 1


def test_scatter_refusals(emu):
    offsets = np.array([0, 5], dtype=np.uint64)
    kstart = np.zeros(1, dtype=np.uint32)
    words = np.zeros((5, 2), dtype=np.uint64)
    roots = np.zeros((4, 4), dtype=np.uint64)
    cnt = np.zeros(8, dtype=np.uint32)

    def run(F=2, bpf=16, cap=10, stride=4, bins=4, n_counts=8):
        return emu.emu_entries_scatter(vp(words), vp(offsets), vp(kstart), C.c_uint32(1), C.c_uint32(F), C.c_uint32(bpf), C.c_uint32(F * bpf), C.c_uint32(cap),
                                       C.c_uint32(0), C.c_uint32(stride), C.c_uint32(bins), vp(roots), vp(cnt), C.c_uint32(n_counts), C.c_uint32(0))
    assert run() == -1 and b"longer than stride" in emu.emu_last_error()
    assert run(cap=4) >= 1
    assert run(cap=4, F=5, bins=4) == -1 and b"more bins" in emu.emu_last_error()
    assert run(cap=4, F=3, bpf=64, bins=4) == -1 and b"out of range" in emu.emu_last_error()
    assert run(cap=0) == -1 and b"out of range" in emu.emu_last_error()


# ------------------------------------------------------------------------------------------------------------- refusals of the plan
def test_bulk_plan_refusals(emu):
    def run(offsets, T, ipb, max_items):
        offsets = np.array(offsets, dtype=np.uint64)
        out = [np.zeros(16, dtype=np.uint32), np.zeros(16, dtype=np.uint32)]
        total = C.c_uint64()
        rc = emu.emu_bulk_plan(vp(offsets), C.c_uint64(T), C.c_uint32(ipb), C.c_uint32(max_items), vp(out[0]), vp(out[1]), C.byref(total))
        return rc, emu.emu_last_error().decode()
    assert run([0, 1, 2, 3, 4], 4, 2, 2)[0] == 0
    for max_items in (0, 1):                                 # cap would be 0
        rc, why = run([0, 1, 2, 3, 4], 4, 2, max_items)
        assert rc == -1 and "max_items_per_bin" in why
    rc, why = run([0, 3, 2, 3, 4], 4, 2, 5)
    assert rc == -1 and "decrease at location 1" in why
    for T, ipb in ((4, 3), (3, 2), (4, 0)):                  # T is not bundle_idx_count * items_per_bundle
        rc, why = run([0, 1, 2, 3, 4], T, ipb, 5)
        assert rc == -1 and "items_per_bundle" in why
    rc, why = run([0, 1 << 32, (1 << 32) + 1], 2, 2, 5)
    assert rc == -1 and "2^32 - 1" in why
    assert run([7, 7 + (1 << 32) - 1, 7 + (1 << 32)], 2, 2, 1 << 31)[0] == 0      # 2^32 - 1 entries is the most
