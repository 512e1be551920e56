"""The plain-Python model of a split (apsu_amd/csrc/bin_split.h) that both tiers are held to: split_cut and slicing of sorted(), the
arrays k_roots_split starts from (the distinct roots in arrival order, found, mult as launch_roots_mult leaves them) and the arrays it
must leave, poison included.  tests/test_bundle_split_cpu.py runs the cases through the CPU emulation, tests/test_gpu_bundle_split.py
through the ROOTS_SPLIT step on the GPU."""
import numpy as np

NONE = 0xFFFFFFFF                                         # LOOKUP_NONE: the slot is not a bin
POISON = 0xEEEEEEEEEEEEEEEE
POISON32 = 0xEEEEEEEE
NO_FAILURE = (1 << 64) - 1
CAPS = (256, 2048, 8192)                                  # the instances' capacities


def cut(c, k, p):
    return p * c // k


def parts_needed(max_count, limit):
    """the smallest k >= 1 with ceil(max_count / k) < limit"""
    k = 1
    while -(-max_count // k) >= limit:
        k += 1
    return k


def split_bins(bins, k):
    """bins: per slot a list of items or None -> k lists of the same shape, part p holding the positions [cut(p), cut(p + 1)) of sorted()"""
    out = []
    for p in range(k):
        out.append([None if b is None else sorted(int(v) for v in b)[cut(len(b), k, p):cut(len(b), k, p + 1)] for b in bins])
    return out


class Bin:
    """one occupied bin as the root search leaves it: `values` distinct, in arrival order; mult per value (None: never written, the
    kernel must take 1 and may not read it); found / count default to what the lists say"""
    def __init__(self, slot, values, mult=None, found=None, count=None):
        self.slot, self.values, self.mult = slot, [int(v) for v in values], mult
        self.found = len(values) if found is None else found
        ms = [1] * len(values) if mult is None else mult
        self.count = sum(ms) if count is None else count

    def total(self):
        ms = [1] * len(self.values) if (self.mult is None or self.found >= self.count) else self.mult
        return sum(ms[:min(self.found, self.count)])

    def ok(self):
        return self.found <= self.count and self.total() == self.count

    def items(self):
        ms = [1] * len(self.values) if (self.mult is None or self.found >= self.count) else self.mult
        out = []
        for v, m in zip(self.values[:self.found], ms):
            out += [v] * m
        return sorted(out)


def from_multiset(slot, items, order="asc", rng=None):
    """a consistent Bin from a multiset: distinct values in the given arrival order, multiplicities where there is a deficit"""
    items = sorted(int(v) for v in items)
    vals = sorted(set(items))
    if order == "desc":
        vals = vals[::-1]
    elif order == "shuffle":
        vals = [vals[i] for i in rng.permutation(len(vals))]
    mult = [items.count(v) for v in vals] if len(vals) < len(items) else None
    return Bin(slot, vals, mult)


class Case:
    """n slots; bins: the occupied ones (count >= 1), ascending slots; empty: slots that are bins of count 0; every other slot is not a bin"""
    def __init__(self, name, n, hstride, k, bins, empty=()):
        self.name, self.n, self.hstride, self.k = name, n, hstride, k
        self.bins = sorted(bins, key=lambda b: b.slot)
        self.counts = np.full(n, NONE, dtype=np.uint32)
        for s in empty:
            self.counts[s] = 0
        for b in self.bins:
            self.counts[b.slot] = b.count
        # one word of room behind the fullest row of every part, so that a write behind a count is seen
        self.stride = [1 + max([cut(b.count, k, p + 1) - cut(b.count, k, p) for b in self.bins] + [0]) for p in range(k)]
        self.off = [0]
        for p in range(k):
            self.off.append(self.off[-1] + n * self.stride[p])

    def inputs(self):
        n_occ, h = len(self.bins), self.hstride
        hits = np.full((n_occ, h), POISON, dtype=np.uint64)
        mult = np.full((n_occ, h), POISON32, dtype=np.uint32)
        found = np.zeros(n_occ, dtype=np.uint32)
        for r, b in enumerate(self.bins):
            found[r] = b.found
            w = min(len(b.values), b.count, h)             # the search writes no value at or behind the count
            hits[r, :w] = np.array(b.values[:w], dtype=np.uint64)
            if b.mult is not None and b.found < b.count:
                mult[r, :len(b.mult)] = np.array(b.mult, dtype=np.uint32)
        occ = np.array([b.slot for b in self.bins], dtype=np.uint32)
        return hits, found, mult, occ

    def expected(self):
        """-> out (the parts' arrays, poison where nothing is written), counts_out [k][n], failure"""
        out = np.full(self.off[-1], POISON, dtype=np.uint64)
        counts_out = np.zeros((self.k, self.n), dtype=np.uint32)
        failure = NO_FAILURE
        for b in self.bins:
            if not b.ok():
                failure = min(failure, b.slot << 32 | (b.found if b.found > b.count else b.total()))
                continue
            items = b.items()
            for p in range(self.k):
                part = items[cut(b.count, self.k, p):cut(b.count, self.k, p + 1)]
                at = self.off[p] + b.slot * self.stride[p]
                out[at:at + len(part)] = np.array(part, dtype=np.uint64)
                counts_out[p, b.slot] = len(part)
        return out, counts_out, failure


def adversarial_cases(t, n=64):
    """the lists of the issue, for a plain modulus t and n slots"""
    rng = np.random.default_rng(20240607)
    cases = []

    def draw(c, distinct=True):
        if distinct:
            return [int(v) for v in rng.choice(min(t, 1 << 20), size=c, replace=False)]
        return [int(v) for v in rng.integers(0, min(t, 40), size=c)]

    for k in (1, 2, 3):
        for order in ("asc", "desc", "shuffle"):
            items = draw(37)
            cases.append(Case("order-%s-k%d" % (order, k), n, 40, k, [from_multiset(5, items, order, rng), from_multiset(n - 1, draw(9), order, rng)], empty=(0, 7)))
    cases.append(Case("all-equal", n, 16, 3, [from_multiset(2, [77] * 11)]))                       # one root of multiplicity c
    cases.append(Case("all-equal-k-c", n, 16, 11, [from_multiset(2, [77] * 11)]))
    cases.append(Case("spans-three-parts", n, 16, 5, [from_multiset(9, [3, 8, 8, 8, 8, 8, 8, 8, 20, 21], "desc")]))   # cuts at 2, 4, 6, 8
    cases.append(Case("root-0-and-t-1", n, 8, 2, [from_multiset(0, [0, t - 1, 5, 0, t - 1], "desc"), from_multiset(1, [t - 1]), from_multiset(63, [0])]))
    cases.append(Case("found-1", n, 4, 2, [from_multiset(3, [123456 % t])]))
    cases.append(Case("k-equals-c", n, 16, 13, [from_multiset(4, draw(13), "shuffle", rng), from_multiset(6, draw(5), "desc")]))   # a bin of count below k
    cases.append(Case("counts-below-k", n, 8, 7, [from_multiset(s, draw(1 + s % 6), "desc") for s in (1, 2, 3, 10, 11, 12)], empty=(0,)))
    cases.append(Case("repeats", n, 64, 3, [from_multiset(s, draw(50, False), "shuffle", rng) for s in (0, 31, 32, 33)]))
    # the refusals: a total above and below the count, found above the count; the bins next to them are served
    good = from_multiset(8, draw(6), "desc")
    cases.append(Case("total-above", n, 8, 2, [Bin(3, [5, 9], mult=[3, 3], count=5), good]))
    cases.append(Case("total-below", n, 8, 2, [Bin(3, [5, 9], mult=[1, 2], count=5), good, Bin(20, [4], mult=[1], count=3)]))
    cases.append(Case("found-above", n, 8, 2, [good, Bin(40, [1, 2, 3], found=5, count=3), Bin(50, [7, 7 + 1], mult=[0, 2], count=2, found=1)]))
    return cases


def boundary_cases(t, n=64):
    """every instance at its capacity, and one entry either side of the boundaries between them"""
    rng = np.random.default_rng(7)
    cases = []
    for h in (255, 256, 257, 2047, 2048, 2049, 8191, 8192):
        top = min(t, 1 << 24)
        vals = [int(v) for v in rng.choice(top, size=min(h, top), replace=False)]
        bins = [from_multiset(1, vals, "shuffle", rng), from_multiset(2, vals[:3] + vals[:2] + vals[:1], "desc")]
        cases.append(Case("hstride-%d" % h, n, h, 3, bins, empty=(0,)))
    return cases
