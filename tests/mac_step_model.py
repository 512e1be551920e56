"""The multiply-accumulate family in Python integers and numpy, and the cases its kernels are run on -- a plain helper module.

Three things, each from its definition and not from apsu_amd/csrc/mac_core.h:

  * sums: exact_chain, sum_t a_t * p_t mod q in Python integers;
  * the row rule: row_bits(q), the smallest w >= max(bits(q), 32) below 64 with (32 - gcd(2 w, 32)) + 2 w <= 128, else 64 -- and
    windows_fit(w, n), that with that w every pair of coefficients lies inside the 16 bytes that start at the dword holding its first bit;
  * the layout: coefficient c of limb j occupies bits [c w_j, (c + 1) w_j) of the little-endian bit string that starts at byte
    row_off[j] of the slot (Rows.pack / Rows.unpack, written from that sentence with numpy's bit arrays).

The cases (MacCase, TermCase) are what BOTH tiers run: tests/test_mac_step_model_cpu.py hands them to the CPU emulation of the
kernels' lanes, tests/test_gpu_mac_steps.py to the gfx950 kernels through apsu_he_debug_run_step's MAC / TERM_PRODUCT steps.  A case
holds the arrays in the step's layout (include/apsu_he.h) and the job fields the step derives from them, so the emulation's job table is
set the same way as the device's."""
import math

import numpy as np

import edge_values as ev

MAC_G = 4
PAD = 16                                                  # bytes the engine keeps readable behind a bit-packed buffer
PATTERN = 0xDEAD00000000BEEF                              # what an output word holds before a launch (no residue: above 2^62)
LONG_CHAIN = 200                                          # widths whose chunk is thousands of terms: one long chain


def chain_lengths(qs):
    """chunk - 2 ... chunk + 2 and 2 chunk + 1 around the two-product and the three-product chunk of the narrowest-chunk limb
    (test_gpu_mac_edges.chain_lengths, restated here so that the CPU tier does not import a GPU test for it)"""
    out = set()
    for c in (min(ev.mac_chunk(q) for q in qs), min(ev.mac_chunk_kara(q) for q in qs)):
        if 0 < c <= 130:
            out |= {c - 2, c - 1, c, c + 1, c + 2, 2 * c + 1}
    return sorted(v for v in out if v >= 1) or [LONG_CHAIN]


# ---------------------------------------------------------------------------------------------------------------- sums
def exact_chain(q, A, P):
    """sum_t A[t] * P[t][p] mod q per coefficient and polynomial p, in Python integers (columns that repeat are computed once)"""
    terms, n = A.shape
    cols = np.concatenate([A, P[:, 0], P[:, 1]])
    mix = np.random.default_rng(1).integers(1, 1 << 63, (3 * terms, 1), dtype=np.uint64) | np.uint64(1)
    _, first, inv = np.unique((cols * mix).sum(axis=0, dtype=np.uint64), return_index=True, return_inverse=True)    # columns by a 64-bit mix ...
    uniq = cols[:, first]
    assert (uniq[:, inv] == cols).all()                   # ... which did not merge two different ones
    a, p0, p1 = (uniq[i * terms:(i + 1) * terms].astype(object) for i in range(3))
    r0 = np.array([int(v) % q for v in (a * p0).sum(axis=0)], dtype=np.uint64)
    r1 = np.array([int(v) % q for v in (a * p1).sum(axis=0)], dtype=np.uint64)
    return np.stack([r0[inv], r1[inv]])


# ---------------------------------------------------------------------------------------------------------------- rows
def row_bits(q):
    """width of a bit-packed row of the prime q"""
    for w in range(max(int(q).bit_length(), 32), 64):
        if (32 - math.gcd(2 * w, 32)) + 2 * w <= 128:
            return w
    return 64


def windows_fit(w, n):
    """every pair (k, k + 1), k even, of a row of n w-bit coefficients fits the 16 bytes from the dword that holds the pair's first bit"""
    return all((k // 2 * 2 * w) % 32 + 2 * w <= 128 for k in range(0, n, 2))


def mask_hi(w, s):
    """what cuts the high half (above the s-bit low half) out of a w-bit coefficient; 64-bit rows need none"""
    return 0xFFFFFFFF if w == 64 else (1 << (w - s)) - 1


class Rows:
    """the bit-packed slot of a level: limb j a row of n coefficients of bits[j] bits, rows back to back"""

    def __init__(self, qs, n, bits=None):
        self.qs, self.n = [int(q) for q in qs], n
        self.bits = list(bits) if bits is not None else [row_bits(q) for q in self.qs]
        assert all(n * w % 8 == 0 for w in self.bits)
        self.row_bytes = [n * w // 8 for w in self.bits]
        self.row_off = [sum(self.row_bytes[:j]) for j in range(len(self.bits))]
        self.slot_bytes = sum(self.row_bytes)

    def pack(self, dense):
        """dense [slots][L][n] -> uint8 [slots * slot_bytes]"""
        dense = np.ascontiguousarray(dense, dtype="<u8")
        slots, L, n = dense.shape
        assert (L, n) == (len(self.bits), self.n)
        out = np.zeros((slots, self.slot_bytes), dtype=np.uint8)
        for j, w in enumerate(self.bits):
            assert not (dense[:, j] >> np.uint64(w)).any() if w < 64 else True
            bits = np.unpackbits(dense[:, j].reshape(slots, n, 1).view(np.uint8), axis=2, bitorder="little")     # [slots][n][64], bit b of coefficient c
            string = bits[:, :, :w].reshape(slots, n * w)                                                        # coefficient c at bits [c w, (c + 1) w)
            out[:, self.row_off[j]:self.row_off[j] + self.row_bytes[j]] = np.packbits(string, axis=1, bitorder="little")
        return out.reshape(-1)

    def unpack(self, packed, slots):
        """uint8 [slots * slot_bytes] (more bytes may follow) -> dense [slots][L][n]"""
        packed = np.ascontiguousarray(packed).view(np.uint8).reshape(-1)[:slots * self.slot_bytes].reshape(slots, self.slot_bytes)
        out = np.zeros((slots, len(self.bits), self.n), dtype=np.uint64)
        for j, w in enumerate(self.bits):
            string = np.unpackbits(packed[:, self.row_off[j]:self.row_off[j] + self.row_bytes[j]], axis=1, bitorder="little")
            bits = np.zeros((slots, self.n, 64), dtype=np.uint8)
            bits[:, :, :w] = string.reshape(slots, self.n, w)
            out[:, j] = np.packbits(bits, axis=2, bitorder="little").view("<u8").reshape(slots, self.n)
        return out

    def words(self, dense, pad=False):
        """the packed slots as the 64-bit words they travel in; pad: with PAD bytes of 0xA5 behind them"""
        b = self.pack(dense)
        if pad:
            b = np.concatenate([b, np.full(PAD, 0xA5, dtype=np.uint8)])
        assert b.size % 8 == 0
        return np.ascontiguousarray(b).view("<u8").copy()


# ---------------------------------------------------------------------------------------------------------------- cases
class MacCase:
    """One launch of k_mac in the MAC step's layout: `batch` jobs over the L limbs qs of a level,
         powers [batch][terms][2][P][n]   (limbs L .. P - 1 hold words no job may read)
         coeffs [batch][polys][terms][L][n]   the plaintexts, dense; packed: Rows(qs, n).words(...) of them
         out0   [batch][polys][2][NL][n]      PATTERN
       and per job (limb0, nl, ng, cnt): the job multiplies limbs limb0 .. limb0 + nl - 1 of its first ng streams over its first cnt
       terms and writes them as limbs 0 .. nl - 1.  table: whether the step is given the job table (else every job is (limb0, NL, polys, terms))."""

    def __init__(self, name, qs, n, P, NL, polys, terms, jobs, powers, coeffs, table):
        self.name, self.qs, self.n, self.P, self.NL, self.polys, self.terms = name, [int(q) for q in qs], n, P, NL, polys, terms
        self.jobs, self.powers, self.coeffs, self.table = jobs, powers, coeffs, table
        self.batch, self.L = len(jobs), len(qs)
        assert powers.shape == (self.batch, terms, 2, P, n) and coeffs.shape == (self.batch, polys, terms, self.L, n)
        for limb0, nl, ng, cnt in jobs:
            assert limb0 + nl <= self.L <= P and 1 <= nl <= NL and 1 <= ng <= polys <= MAC_G and 1 <= cnt <= terms
            assert table or (nl, ng, cnt) == (NL, polys, terms)
        assert table or len({j[0] for j in jobs}) == 1

    def out0(self):
        return np.full((self.batch, self.polys, 2, self.NL, self.n), PATTERN, dtype=np.uint64)

    def job_table(self):
        return np.array(self.jobs, dtype=np.uint64) if self.table else None

    def expected(self):
        """out0 with every (job, stream, handled limb) replaced by its exact sums; computed once"""
        if not hasattr(self, "_exp"):
            exp = self.out0()
            for b, (limb0, nl, ng, cnt) in enumerate(self.jobs):
                for g in range(ng):
                    for i in range(nl):
                        j = limb0 + i
                        exp[b, g, :, i] = exact_chain(self.qs[j], self.coeffs[b, g, :cnt, j], self.powers[b, :cnt, :, j])
            self._exp = exp
        return self._exp

    def wrong(self, out):
        """[(job, stream, polynomial, limb)] of the rows of `out` that differ from expected(), untouched rows included"""
        bad = np.argwhere((np.asarray(out).reshape(self.expected().shape) != self.expected()).any(axis=4))
        return [tuple(int(v) for v in r) for r in bad]


def make_case(name, qs, n, jobs, seed, P=None, NL=None, polys=None, terms=None, table=True, turn=0):
    """the arrays of a MacCase: job x's powers are one polynomial pair of edge_values.FILLS[(x + turn) % 4] rotated per term, stream g's
    coefficients one polynomial of FILLS[(x + turn + g + 1) % 4] rotated per term, and one coefficient that no other stream of the job has.  Terms and streams a job does not use hold canonical data of their own; limbs L .. P - 1 of the powers hold
    0xEE.. words (no residue of any modulus)"""
    L = len(qs)
    P = L if P is None else P
    NL = max(j[1] for j in jobs) if NL is None else NL
    polys = max(j[2] for j in jobs) if polys is None else polys
    terms = max(j[3] for j in jobs) if terms is None else terms
    rng = np.random.default_rng(seed)
    powers = np.full((len(jobs), terms, 2, P, n), 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    coeffs = np.empty((len(jobs), polys, terms, L, n), dtype=np.uint64)
    for x in range(len(jobs)):
        pf = ev.FILLS[(x + turn) % 4]
        base = np.stack([ev.fill_poly(pf, qs, n, rng) for _ in range(2)])                           # [2][L][n]
        for t in range(terms):
            powers[x, t, :, :L] = np.roll(base, t % 7, axis=2)
        for g in range(polys):
            one = ev.fill_poly(ev.FILLS[(x + turn + g + 1) % 4], qs, n, rng)
            for t in range(terms):
                coeffs[x, g, t] = np.roll(one, (t + 3 * g) % 5, axis=1)
            coeffs[x, g, jobs[x][3] // 2, :, (g * 37) % n] = [q - 1 - g for q in qs]                # no two streams of a job hold the same data
    return MacCase(name, qs, n, P, NL, polys, terms, [tuple(j) for j in jobs], powers, coeffs, table)


def worst_case_launches(qs, n, seed, lengths=None):
    """the worst-case chains of a level as launches of three jobs: one job per chain length -- chain_lengths(qs) around either form's
    chunk, or one long chain, and 1, 2, 3 terms (the clamped prefetch of the ping-pong) -- with 1, 3, 4 streams in turn over every limb,
    every operand an extreme: both operands go through all four fills of edge_values.  Lengths are sorted, so a launch's arrays are as long as its longest chain, not the level's."""
    L = len(qs)
    lengths = sorted(set(chain_lengths(qs) if lengths is None else lengths) | {1, 2, 3})
    out = []
    for x0 in range(0, len(lengths), 3):
        jobs = [(0, L, (1, 3, 4)[(x0 + i) % 3], cnt) for i, cnt in enumerate(lengths[x0:x0 + 3])]
        out.append(make_case("chains %s" % [j[3] for j in jobs], qs, n, jobs, [seed, x0], polys=4, turn=x0))    # job x0 + i: fill (x0 + i) % 4
    assert {j[2] for c in out for j in c.jobs} == {1, 3, 4} and len(lengths) >= 4                                  # every stream count, every fill of the powers
    return out


def limb_windows(L):
    """the (limb0, nl) a job is directed at: every limb, all but the last (the engine's nl = Lh over Ll = Lh + 1), all but the first, the last alone"""
    return sorted({(0, L), (0, L - 1), (1, L - 1), (L - 1, 1)} - {(0, 0), (1, 0)})


def directed_launches(qs, n, seed):
    """limb windows and strides: for each (limb0, nl) of limb_windows and P = L, L + 3 a launch WITHOUT a job table (two jobs, two
    streams, three terms; out_poly_stride = nl n, pw_poly_stride = P n, pt_stride = a slot: all three differ for nl < L < P); then one
    launch WITH a table of jobs whose (limb0, nl), stream counts and chain lengths all differ over outputs of NL = L limbs and four
    streams, so that some workgroups leave at b_limb >= nl, some streams are not the job's, and what a job does not own keeps its pattern"""
    L = len(qs)
    out = []
    for limb0, nl in limb_windows(L):
        for P in (L, L + 3):
            out.append(make_case("limb0 %d nl %d P %d" % (limb0, nl, P), qs, n, [(limb0, nl, 2, 3)] * 2, [seed, limb0, nl, P], P=P, table=False, turn=len(out)))
    table = [(limb0, nl, ng, cnt) for (limb0, nl), ng, cnt in zip(limb_windows(L) + [(min(1, L - 1), 1), (0, 1)], (1, 2, 3, 4, 2, 1), (1, 2, 3, 5, 4, 7))]
    assert L >= 3 and len({t[:2] for t in table}) >= 5
    for P in (L, L + 3):
        out.append(make_case("job table P %d" % P, qs, n, table, [seed, 99, P], P=P, NL=L, polys=4))
    return out


class TermCase:
    """One launch of k_term_product on limb `limb` in the TERM_PRODUCT step's layout: `batch` operand sets, each repeated `repeat` times;
    job u reads set u % batch.  powers [batch][2][P][n], coeffs [batch][L][n] -> out [batch * repeat + 1][2][n], the last [2][n] a guard"""

    def __init__(self, qs, n, limb, batch, repeat, seed, P=None):
        L = len(qs)
        self.qs, self.n, self.limb, self.batch, self.repeat, self.L = [int(q) for q in qs], n, limb, batch, repeat, L
        self.P = L if P is None else P
        rng = np.random.default_rng(seed)
        self.powers = np.full((batch, 2, self.P, n), 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
        for b in range(batch):
            for p in range(2):
                self.powers[b, p, :L] = ev.fill_poly(("alternating", "max_halves", "q-1")[(b + p) % 3], qs, n, rng)
        self.coeffs = np.stack([ev.fill_poly(("sprinkled", "max_halves", "q-1", "alternating")[b % 4], qs, n, rng) for b in range(batch)])
        self.njobs = batch * repeat

    def out0(self):
        return np.full((self.njobs + 1, 2, self.n), PATTERN, dtype=np.uint64)

    def expected(self):
        if not hasattr(self, "_exp"):
            q = self.qs[self.limb]
            sets = np.stack([exact_chain(q, self.coeffs[b, self.limb][None], self.powers[b, :, self.limb][None]) for b in range(self.batch)])
            exp = self.out0()
            exp[:self.njobs] = sets[np.arange(self.njobs) % self.batch]
            self._exp = exp
        return self._exp

    def as_mac_case(self):
        """the same operands as chains of one term: job b = set b, one stream, limb `limb` alone"""
        return MacCase("term as chain", self.qs, self.n, self.P, 1, 1, 1, [(self.limb, 1, 1, 1)] * self.batch,
                       np.ascontiguousarray(self.powers[:, None]), np.ascontiguousarray(self.coeffs[:, None, None]), False)


# ---------------------------------------------------------------------------------------------------------------- the chains both tiers run
# name -> bit sizes of the coefficient primes (the last one is the special prime: a level has the others).  Equal widths, one context
# each; "mixed": the data limbs' widths all differ, 51 bits are stored in 52 and 55 in 56, and in this order limb 1 and limb 2 start at
# byte offsets n (33) / 8 and n (33 + 52) / 8 of the slot, which at n = 64 are 8 modulo 16 (at n = 1024 every row is a multiple of
# 128 bytes long, whatever the order); "36-36-60": two narrow limbs and a 64-bit row in one slot.
CHAINS = {"24x3": [24] * 3, "32x3": [32] * 3, "36x3": [36] * 3, "48x3": [48] * 3, "49x3": [49] * 3, "50x3": [50] * 3, "52x3": [52] * 3,
          "56x4": [56] * 4, "58x3": [58] * 3, "60x3": [60] * 3, "mixed": [33, 51, 49, 55, 60], "36-36-60": [36, 36, 60, 60]}
STORED = {"24x3": [32] * 2, "32x3": [32] * 2, "36x3": [36] * 2, "48x3": [48] * 2, "49x3": [49] * 2, "50x3": [50] * 2, "52x3": [52] * 2,
          "56x4": [56] * 3, "58x3": [64] * 2, "60x3": [64] * 2, "mixed": [33, 52, 49, 56], "36-36-60": [36, 36, 64]}
EQUAL_CHAINS = [c for c in CHAINS if c[0].isdigit() and "-" not in c]
DIRECTED_CHAINS = ["mixed", "56x4"]


def chain(name, n):
    """(the coefficient primes, the plain modulus, the limbs of the first data level) of a chain at ring size n"""
    from oracle import pymodel
    q = pymodel.coeff_modulus_create(n, CHAINS[name])
    assert [v.bit_length() for v in q] == CHAINS[name]
    return q, pymodel.coeff_modulus_create(n, [17])[0], len(q) - 1
