"""Hand-built collision cases for the cuckoo table rule, shared by the CPU tier (test_cuckoo_cpu.py) and the GPU (test_gpu_cuckoo.py).
A case: (name, items uint8 [count][16], locs uint32 [count][H], H, T, max_rounds, succeeds).  The locations are GIVEN, not hashed: no item
set steers collisions like these."""
import numpy as np


def _items(tags):
    """one distinct 16-byte item per distinct tag"""
    out = np.zeros((len(tags), 16), dtype=np.uint8)
    for i, t in enumerate(tags):
        out[i] = np.frombuffer(int(t * 0x9E3779B97F4A7C15 + 1).to_bytes(16, "little"), dtype=np.uint8)
    return out


def _case(name, tags, locs, T, max_rounds=500, succeeds=True):
    locs = np.array(locs, dtype=np.uint32).reshape(len(tags), -1) if len(tags) else np.zeros((0, 3), dtype=np.uint32)
    return (name, _items(tags), locs, locs.shape[1], T, max_rounds, succeeds)


def collision_cases():
    far = list(range(1, 200))
    rng = np.random.default_rng(0x435543)
    far_locs = [[int(v) for v in rng.integers(0, 1024, 3)] for _ in range(len(far))]
    return [
        _case("no items", [], [], 4),
        _case("one item", [1], [[2, 0, 1]], 3),
        _case("one slot", [1], [[0]], 1),
        _case("two items, one location list", [1, 2], [[1, 2, 3], [1, 2, 3]], 4),
        # round 0: A and C and D sit, B loses slot 0; round 1: B takes C's slot 2; round 2: C takes D's slot 3; round 3: D goes to 4
        _case("eviction chain", [1, 2, 3, 4], [[0, 1], [0, 2], [2, 3], [3, 4]], 5),
        _case("three items on two locations", [1, 2, 3], [[0, 1], [0, 1], [0, 1]], 2, max_rounds=16, succeeds=False),
        _case("the last round places", [1, 2], [[0, 1], [0, 1]], 2, max_rounds=2),
        _case("one round too few", [1, 2], [[0, 1], [0, 1]], 2, max_rounds=1, succeeds=False),
        _case("adjacent duplicates", [1, 1, 2], [[3, 4, 5], [3, 4, 5], [3, 0, 1]], 6),
        _case("duplicates far apart", far + [far[0]], far_locs + [far_locs[0]], 1024),
        _case("a triple", [7, 7, 7], [[1, 0, 2]] * 3, 3),
        # X (items 0, 1) sits in slot 1; W beats Z in slot 5, Z moves to slot 1 in round 1 and evicts X, which moves on; item 1 stays a duplicate
        _case("duplicate of an item evicted later", [1, 1, 2, 3], [[1, 2], [1, 2], [5, 6], [5, 1]], 7),
        _case("functions that collide on one location", [1, 2], [[2, 2, 2], [2, 2, 0]], 3),
    ]


def random_case(count, T, H, seed, duplicates=0):
    """random locations, `duplicates` of the items repeated (with their location lists) at random places"""
    rng = np.random.default_rng(seed)
    items = rng.integers(0, 256, (count, 16), dtype=np.uint8)
    locs = rng.integers(0, T, (count, H)).astype(np.uint32)
    for _ in range(duplicates):
        a, b = (int(v) for v in rng.integers(0, count, 2))
        items[b] = items[a]
        locs[b] = locs[a]
    return ("%d random items in %d slots" % (count, T), items, locs, H, T, 500, True)
