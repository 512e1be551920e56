"""The querier-side and decryption steps of apsu_he_debug_run_step (seed_expand .. flag_monomial; apsu_amd/csrc/engine_query_steps.cpp) on
Python integers, each from the definition of the step -- nothing here is derived from the kernels.  tests/test_query_step_model_cpu.py
holds it to things it did not come from (the host codec's sampler, the C oracle's decrypt and add_plain, the emulation's samplers and
rounding); tests/test_gpu_query_steps.py holds the kernels to it, bit for bit.  The random streams are query_side_model.py's.

Also the one copy of SEAL's generator as a stream of 64-bit words and of util::sample_poly_uniform that test_seal_codec.py uses."""
import hashlib
import struct

import numpy as np

import query_side_model as M
from oracle.blake2x import blake2xb

W64 = 1 << 64
SEED_REJ_CAP = 8192                       # rejected positions per object the device list holds as compiled


# ---------------------------------------------------------------------------------------------- the generators
def prng_words(seed):
    """SEAL's Blake2xb generator as a stream of 64-bit words"""
    key = struct.pack("<8Q", *[int(w) for w in seed])
    counter = 0
    while True:
        buf = blake2xb(4096, struct.pack("<Q", counter), key)
        counter += 1
        yield from struct.unpack("<512Q", buf)


def shake_words(seed):
    """SEAL's Shake256 generator [SEAL-recall]: 4096-byte buffer k = SHAKE256(seed || k as u64), python's hashlib as the pin of SHAKE256"""
    key = struct.pack("<8Q", *[int(w) for w in seed])
    counter = 0
    while True:
        buf = hashlib.shake_256(key + struct.pack("<Q", counter)).digest(4096)
        counter += 1
        yield from struct.unpack("<512Q", buf)


def max_multiple(q):
    """util/rlwe.cpp: a word at or above it is rejected"""
    return (W64 - 1) - ((W64 - 1) % q) - 1


def sample_poly_uniform(seed, q, n, shake=False):
    g = shake_words(seed) if shake else prng_words(seed)
    L = len(q)
    out = np.array([next(g) for _ in range(L * n)], dtype=object).reshape(L, n)
    for j, qj in enumerate(q):
        mm = max_multiple(qj)
        for k in range(n):
            r = out[j, k]
            while r >= mm:
                r = next(g)
            out[j, k] = r % qj
    return out.astype(np.uint64)


def bulk_words(seed, count):
    """the generator's first `count` words: the ones the bulk pass of the expansion reads"""
    g = prng_words(seed)
    return [next(g) for _ in range(count)]


# ---------------------------------------------------------------------------------------------- seed_expand
def high_rejection_primes(n, count):
    """`count` 60-bit primes = 1 mod 2n just above 2^64 / 17: 16 q < 2^64 < 17 q leaves 2^64 - 16 q, nearly q, above the largest multiple
    of q, so about one word in 17 is refused.  SEAL's own primes sit just below a power of two, 2^b - c, where the same zone is
    2^(64 - b) c: they refuse fewer than one word in 2^27, and an object of theirs practically never has two refused words."""
    from oracle.pymodel import is_prime
    out, v = [], (W64 // 17) // (2 * n) * (2 * n) + 1 + 2 * n
    while len(out) < count:
        if is_prime(v):
            out.append(v)
        v += 2 * n
    return out


def rejection_count(seed, q, n):
    """the words of the object's bulk pass that SEAL's thresholds refuse: what its device list has to hold"""
    th = [max_multiple(int(v)) for v in q]
    return sum(1 for w, x in enumerate(bulk_words([int(v) for v in seed], len(q) * n)) if x >= th[w // n])


def seed_expand(seed, q, n, thresholds=None, cap=SEED_REJ_CAP):
    """sample_poly_uniform with the caller's thresholds (default: SEAL's) and a list cap -> (words, rejected, count, overflowed).
    words [L][n] Python integers; rejected [L][n] bool: the positions whose first word was refused; count = their number.
    count <= cap: every position holds its word (a refused one the next word of the stream, in position order, that passes its limb's
    threshold).  count > cap: overflowed, the refused positions are not written (None) and the rest are."""
    L = len(q)
    th = [max_multiple(v) for v in q] if thresholds is None else [int(v) for v in thresholds]
    g = prng_words(seed)
    raw = [next(g) for _ in range(L * n)]
    rejected = np.array([raw[w] >= th[w // n] for w in range(L * n)], dtype=bool).reshape(L, n)
    count = int(rejected.sum())
    overflowed = count > cap
    out = np.empty((L, n), dtype=object)
    for w in range(L * n):
        j, k = divmod(w, n)
        r = raw[w]
        if rejected[j, k]:
            if overflowed:
                out[j, k] = None
                continue
            while r >= th[j]:
                r = next(g)
        out[j, k] = r % q[j]
    return out, rejected, count, overflowed


# ---------------------------------------------------------------------------------------------- decryption
def decrypt_round(x, q0, t):
    """-> (m, r): m = round(t x / q0) mod t with halves up, r = t x mod q0"""
    return ((x * t + q0 // 2) // q0) % t, x * t % q0


def distance(r, q0):
    return min(r, q0 - r)


def decrypt_round_poly(c0, v, q0, t):
    """c0, v: [n] integers below q0 -> (m [n], worst)"""
    out, worst = [], 0
    for a, b in zip(c0, v):
        m, r = decrypt_round((int(a) + int(b)) % q0, q0, t)
        out.append(m)
        worst = max(worst, distance(r, q0))
    return out, worst


def budget_bits(worst, q0):
    """the largest b with worst 2^b < q0; the bit count of q0 for worst = 0"""
    if worst == 0:
        return q0.bit_length()
    b = 0
    while worst << (b + 1) < q0:
        b += 1
    return b


# ---------------------------------------------------------------------------------------------- the querier's side
def slot_map(n):
    """BatchEncoder's index map: slot value i goes to coefficient-side position map[i] in front of the inverse transform mod t"""
    logn, m = n.bit_length() - 1, 2 * n
    brv = lambda x: int(format(x, "0%db" % logn)[::-1], 2)
    mp, pos = [0] * n, 1
    for i in range(n // 2):
        mp[i] = brv((pos - 1) >> 1)
        mp[n // 2 + i] = brv((m - pos - 1) >> 1)
        pos = pos * 3 % m
    return mp


def plain_powers(vals, exps, t, n):
    """vals [batch][n] any 64-bit words -> (out [batch * S][n], flag): out[b S + s][slot_map[i]] = vals[b][i]^exps[s] mod t, a value >= t
    counting as 0 and raising the flag; 0^0 = 1"""
    mp = slot_map(n)
    S = len(exps)
    out = np.zeros((len(vals) * S, n), dtype=object)
    flag = 0
    for b, row in enumerate(vals):
        for i, x in enumerate(row):
            x = int(x)
            if x >= t:
                flag, x = 1, 0
            for s, e in enumerate(exps):
                out[b * S + s, mp[i]] = pow(x, int(e), t)
    return out, flag


def secret(seed, n):
    return M.secret(seed, n)


def noise(seed, first_object, count, n):
    return np.stack([M.noise(seed, first_object + c, n) for c in range(count)])


def small_lift(small, q):
    """small [batch][n] signed -> [batch][len(q)][n] residues"""
    return np.array([[[int(v) % m for v in row] for m in q] for row in small], dtype=object)


def delta(m, q, t):
    """SEAL's scaling of a plaintext coefficient at the level with moduli q: round(m Q / t) = floor((m Q + floor((t + 1) / 2)) / t)"""
    Q = 1
    for v in q:
        Q *= v
    return (int(m) * Q + (t + 1) // 2) // t


def enc_finish(pt, v, e, q, t):
    """pt [n] mod t, v [L][n], e [n] signed -> c0 [L][n]: c0_j = Delta(m) - e - v_j mod q_j"""
    return np.array([[(delta(m, q, t) - int(ek) - int(vj[k])) % qj for k, (m, ek) in enumerate(zip(pt, e))] for vj, qj in zip(v, q)], dtype=object)


def rlk_finish(a, s, e, key_q):
    """a [K - 1][K][n], s [K][n], e [K - 1][K][n] -> c0 [K - 1][K][n]: c0[i][j] = -(a[i][j] s_j + e[i][j]) + [j == i] (p mod q_i) s_i^2 mod q_j,
    p the last (special) prime"""
    K, p = len(key_q), key_q[-1]
    out = np.empty((K - 1, K, len(s[0])), dtype=object)
    for i in range(K - 1):
        for j, q in enumerate(key_q):
            for k in range(len(s[0])):
                sk = int(s[j][k])
                r = -(int(a[i][j][k]) * sk + int(e[i][j][k]))
                if j == i:
                    r += (p % q) * sk * sk
                out[i, j, k] = r % q
    return out


def flag_monomial(pt):
    """pt [batch][n] -> [batch]: 1 where exactly one word is non-zero"""
    return [1 if sum(1 for w in row if int(w) != 0) == 1 else 0 for row in pt]


# ---------------------------------------------------------------------------------------------- the directed cases both test files use
def seed_of(label):
    """a 64-byte seed as eight words, named by a label"""
    return list(struct.unpack("<8Q", hashlib.blake2b(label.encode(), digest_size=64).digest()))


def kth_largest(words, k):
    """the threshold that refuses exactly k of `words` (they are distinct, which the CPU tests confirm through the counts)"""
    return sorted(words, reverse=True)[k - 1]


class SeedCase:
    """one seed_expand launch: `limbs` of n words per object, one seed per object, thresholds [limbs], the list cap"""

    def __init__(self, name, n, limbs, seeds, thresholds, cap, counts):
        self.name, self.n, self.limbs, self.seeds, self.cap = name, n, limbs, seeds, cap
        self.thresholds = [int(v) for v in thresholds]
        self.counts = counts                          # the rejected words of every object, as the case was built to have them

    def expected(self, q):
        """per object (words, rejected, count, overflowed) under the moduli q[:limbs]"""
        return [seed_expand(s, [int(v) for v in q[:self.limbs]], self.n, self.thresholds, self.cap) for s in self.seeds]


NO_REJECTION = W64 - 1
EDGE_SEED = "edge-4876"        # found by search: words 0 and 127 of its stream are the largest of words 0 .. 63 and 64 .. 127


def seed_cases_small(n=64):
    """the cases at n = 64 (levels of 1 .. 4 limbs), thresholds and caps chosen from the bulk words so that every count is known"""
    cases = []
    s = seed_of("none")
    cases.append(SeedCase("no rejection", n, 3, [s], [NO_REJECTION] * 3, SEED_REJ_CAP, [0]))
    s = seed_of(EDGE_SEED)
    raw = bulk_words(s, 2 * n)
    cases.append(SeedCase("word 0 and word L n - 1", n, 2, [s], [raw[0], raw[2 * n - 1]], SEED_REJ_CAP, [2]))
    s = seed_of("cap")
    t5 = kth_largest(bulk_words(s, 3 * n), 5)
    cases.append(SeedCase("count == cap", n, 3, [s], [t5] * 3, 5, [5]))
    cases.append(SeedCase("count == cap + 1", n, 3, [s], [t5] * 3, 4, [5]))
    cases.append(SeedCase("cap 1, one rejection", n, 3, [s], [kth_largest(bulk_words(s, 3 * n), 1)] * 3, 1, [1]))
    # three objects under one threshold (1 word in 32 refused); the cap is the second largest count, the largest goes in the middle
    th = W64 - (1 << 59)
    seeds = [seed_of("mixed-%d" % i) for i in range(3)]
    counts = [sum(1 for w in bulk_words(sd, 3 * n) if w >= th) for sd in seeds]
    order = sorted(range(3), key=lambda i: counts[i])
    order = [order[0], order[2], order[1]]
    cases.append(SeedCase("mixed overflow", n, 3, [seeds[i] for i in order], [th] * 3, sorted(counts)[1], [counts[i] for i in order]))
    s = seed_of("redraw")
    cases.append(SeedCase("thresholds at 2^62", n, 3, [s], [1 << 62] * 3, SEED_REJ_CAP, [sum(1 for w in bulk_words(s, 3 * n) if w >> 62)]))
    s = seed_of("per-limb")
    th3 = [W64 - (1 << 60), W64 - (1 << 58), 1 << 63]
    cases.append(SeedCase("a threshold per limb", n, 3, [s], th3, SEED_REJ_CAP, [sum(1 for w, x in enumerate(bulk_words(s, 3 * n)) if x >= th3[w // n])]))
    return cases


def seed_case_key_level(n, K):
    """all K key limbs, 1 word in 16 refused in every limb, two objects"""
    th = W64 - (1 << 60)
    seeds = [seed_of("key-%d-%d" % (K, i)) for i in range(2)]
    return SeedCase("key level", n, K, seeds, [th] * K, SEED_REJ_CAP, [sum(1 for w in bulk_words(sd, K * n) if w >= th) for sd in seeds])


def seed_case_refill(n=1024):
    """one limb of 1024 words under 2^62: three words in four are refused and so are their replacements, so the redraw cursor walks
    through several 64-block (512-word) windows of the stream"""
    s = seed_of("refill")
    return SeedCase("thresholds at 2^62, n = 1024", n, 1, [s], [1 << 62], SEED_REJ_CAP, [sum(1 for w in bulk_words(s, n) if w >> 62)])


def seed_cases_compiled_cap(n=8192, label="compiled-cap"):
    """two limbs of 8192 words: per-limb thresholds from the sorted bulk words so that exactly 8192, then exactly 8193 words are refused"""
    s = seed_of(label)
    raw = bulk_words(s, 2 * n)
    lo, hi = raw[:n], raw[n:]
    t0, t1, t1b = kth_largest(lo, SEED_REJ_CAP // 2), kth_largest(hi, SEED_REJ_CAP // 2), kth_largest(hi, SEED_REJ_CAP // 2 + 1)
    return [SeedCase("8192 refused", n, 2, [s], [t0, t1], SEED_REJ_CAP, [SEED_REJ_CAP]),
            SeedCase("8193 refused", n, 2, [s], [t0, t1b], SEED_REJ_CAP, [SEED_REJ_CAP + 1])]


def decrypt_edges(q0, t):
    """x at the ends of its range and at the rounding's and the centring's boundaries (q0 odd)"""
    import math
    h = q0 >> 1
    xs = [0, 1, q0 - 1, (q0 - 1) // 2, (q0 + 1) // 2]
    if math.gcd(t, q0) == 1:
        inv = pow(t, -1, q0)
        # r = t x mod q0 at 0, 1, either side of the centring, q0 - 1, and where t x + floor(q0 / 2) is 0 and q0 - 1 mod q0
        xs += [r * inv % q0 for r in (0, 1, h, h + 1, q0 - 1, -h % q0, (q0 - 1 - h) % q0)]
    return xs


def decrypt_pairs_fixed():
    """the (q0, t) pairs that do not come from a context: the largest the rounding admits, and the smallest"""
    return [((1 << 62) - 1, (1 << 61) - 1), (3, 2)]
