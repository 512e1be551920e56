"""Model of the engine's cuckoo hashing, written from the contract in include/apsu_he.h and independently of apsu_amd/csrc/cuckoo.h:
the tests hold the CPU tier (libapsu_he_hostemu.so) and the GPU against it bit for bit.

* tables / locations: Kuku 2.x's LocFunc as the header restates it [Kuku-recall] -- tab_f[16][256] little-endian 32-bit words of
  blake2xb(16384, make_item(f, 0)) from the oracle's BLAKE2X model, loc_f(item) = XOR_p tab_f[p][item[p]] mod table_size, in plain
  integers.  UNPINNED like the header's statement: no Kuku source or known-answer vector has been held against it.
* insert: the engine's own table rule as two loops per round over a dict of slots.
* bucket: the database side's grouping, by sorting.
"""
import functools
import glob
import json
import os
import struct

from oracle import blake2x

EMPTY = (1 << 64) - 1
NONE = 0xFFFFFFFF
DEFAULT_ROUNDS = 500


@functools.lru_cache(maxsize=None)
def tables(f):
    """tab_f as a tuple of 16 tuples of 256 ints"""
    raw = blake2x.blake2xb(16384, struct.pack("<QQ", f, 0))
    words = struct.unpack("<4096I", raw)
    return tuple(tuple(words[p * 256:(p + 1) * 256]) for p in range(16))


def location(item, f, table_size):
    item = bytes(item)
    assert len(item) == 16
    x = 0
    tab = tables(f)
    for p in range(16):
        x ^= tab[p][item[p]]
    return x % table_size


def locations(items, hash_func_count, table_size):
    """-> [count][hash_func_count] ints"""
    return [[location(it, f, table_size) for f in range(hash_func_count)] for it in items]


class Table:
    def __init__(self):
        self.ok = False
        self.rounds = 0
        self.unplaced = None        # lowest item without a slot when not ok
        self.table_idx = None       # [T]: item or NONE
        self.item_loc = None        # [count]: location, NONE for a duplicate
        self.fill = 0.0


def insert(items, locs, hash_func_count, table_size, max_rounds=DEFAULT_ROUNDS):
    """items: sequence of 16-byte values (compared for equality only); locs[i][f]: the locations of item i"""
    assert 1 <= max_rounds <= 1 << 32
    count = len(items)
    items = [bytes(it) for it in items]
    slots = {}                      # location -> key
    h = [0] * count
    last_key = [None] * count
    active = list(range(count))
    duplicate = set()
    out = Table()
    for r in range(max_rounds):
        if not active:
            break
        for i in active:            # propose: a minimum, so the order of this loop does not matter
            key = ((max_rounds - 1 - r) << 32) | i
            loc = locs[i][h[i]]
            if key < slots.get(loc, EMPTY):
                slots[loc] = key
            last_key[i] = key
        active = []
        for i in range(count):      # settle
            if i in duplicate:
                continue
            held = slots[locs[i][h[i]]]
            if held == last_key[i]:
                continue
            winner = held & 0xFFFFFFFF
            if items[winner] == items[i]:
                duplicate.add(i)
            else:
                h[i] = (h[i] + 1) % hash_func_count
                active.append(i)
        out.rounds = r + 1
    out.ok = not active
    out.fill = len(slots) / table_size
    if active:
        out.unplaced = min(active)
        return out
    out.table_idx = [NONE] * table_size
    for loc, key in slots.items():
        out.table_idx[loc] = key & 0xFFFFFFFF
    out.item_loc = [NONE if i in duplicate else locs[i][h[i]] for i in range(count)]
    return out


def check_invariants(items, locs, t):
    """one slot per surviving item, the slot one of the item's locations, nothing lost (every item survives or equals a survivor)"""
    items = [bytes(it) for it in items]
    seen = {}
    for i, loc in enumerate(t.item_loc):
        if loc == NONE:
            continue
        assert loc in locs[i] and t.table_idx[loc] == i
        assert items[i] not in seen
        seen[items[i]] = i
    assert sum(1 for v in t.table_idx if v != NONE) == len(seen)
    for i, loc in enumerate(t.item_loc):
        if loc == NONE:
            assert seen[items[i]] < i


def bucket(locs, table_size):
    """-> (offsets [T + 1], order): bucket l holds, in input order, the items with l among their locations, each once"""
    pairs = sorted({(loc, i) for i, li in enumerate(locs) for loc in li})
    offsets = [0] * (table_size + 1)
    for loc, _ in pairs:
        offsets[loc + 1] += 1
    for l in range(table_size):
        offsets[l + 1] += offsets[l]
    return offsets, [i for _, i in pairs]


def shipped_pairs():
    """the (set size, table_size, hash_func_count) triples of the shipped parameter sets, from tests/params (the set size is the second
    field of the file's name)"""
    out = set()
    for p in glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "params", "*.json")):
        with open(p) as f:
            tp = json.load(f)["table_params"]
        out.add((int(os.path.basename(p)[:-5].split("-")[1]), tp["table_size"], tp["hash_func_count"]))
    return sorted(out)
