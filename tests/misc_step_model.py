"""The launchers behind the steps ADD .. PACK_BLOCKS of apsu_he_debug_run_step (apsu_amd/csrc/engine_misc_steps.cpp), stated on Python
integers, and the edge cases of each.  tests/test_misc_step_model_cpu.py holds every model to an independent statement that the tree
already has; tests/test_gpu_misc_steps.py holds the kernels to the models."""
import struct

import numpy as np

from oracle import blake2x

M64 = (1 << 64) - 1
GUARD = 0xA5A5A5A5A5A5A5A5


def u64(x):
    return np.ascontiguousarray(x, dtype=np.uint64)


def obj(x):
    """a numpy array of Python integers"""
    return np.array([int(v) for v in np.asarray(x).reshape(-1)], dtype=object).reshape(np.asarray(x).shape)


# ------------------------------------------------------------------------------------------------------------- ADD, CLEAR_BITS
def add(acc, x, q, n):
    """[..][L][n] words: per limb (acc + x) mod q_j"""
    a, b = obj(acc).reshape(-1, len(q), n), obj(x).reshape(-1, len(q), n)
    return u64(np.stack([(a[:, j] + b[:, j]) % q[j] for j in range(len(q))], axis=1).reshape(np.asarray(acc).shape))


def add_operands(q, n, batch, polys, rng):
    """per limb (q - 1) + (q - 1), (q - 1) + 1, 0 + 0, 1 + (q - 1), then random"""
    a, b = np.zeros((batch * polys, len(q), n), dtype=np.uint64), np.zeros((batch * polys, len(q), n), dtype=np.uint64)
    for j, m in enumerate(q):
        a[:, j], b[:, j] = rng.integers(0, m, (batch * polys, n), dtype=np.uint64), rng.integers(0, m, (batch * polys, n), dtype=np.uint64)
        for r in range(batch * polys):
            k = (3 * r + j) % (n - 3)                           # the edges move along the row: another lane each time
            a[r, j, k:k + 4], b[r, j, k:k + 4] = [m - 1, m - 1, 0, 1], [m - 1, 1, 0, m - 1]
        a[:, j, n - 1], b[:, j, n - 1] = m - 1, m - 1           # the last lane of the last workgroup
    return a, b


def clear_bits(words, bits):
    return u64(words) & np.uint64(M64 ^ ((1 << bits) - 1))


CLEAR_WORDS = [0, 1, M64, 1 << 63, (1 << 63) - 1, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA]


# ------------------------------------------------------------------------------------------------------------- COPY_SOURCES
def sources_report(src, q, n, before, seq):
    """the report word after the launch: max(before, seq) when a word of a job is at or above the prime of its limb ((k / n) % L)"""
    s = obj(src).reshape(-1, 2, len(q), n)
    bad = any((s[:, :, j] >= q[j]).any() for j in range(len(q)))
    return max(before, seq) if bad else before


# ------------------------------------------------------------------------------------------------------------- the generators
GAMMA = 0x9E3779B97F4A7C15


def splitmix64(z):
    """the output function of splitmix64 on the state z (64-bit wrap)"""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def fill_random(words, seed, bound):
    """out[i] = splitmix64(seed + (i + 1) gamma) % bound, as k_fill_random's comment documents it"""
    return u64([splitmix64((seed + (i + 1) * GAMMA) & M64) % bound for i in range(words)])


_BUFFERS = {}


def blake_value(seed, g):
    """the g-th 32-bit output of SEAL's Blake2xb generator: value g % 1024 of buffer g // 1024, blake2xb(4096, counter, key = seed)"""
    key = (bytes(seed), g // 1024)
    if key not in _BUFFERS:
        _BUFFERS[key] = blake2x.blake2xb(4096, struct.pack("<Q", g // 1024), bytes(seed))
    return struct.unpack_from("<I", _BUFFERS[key], (g % 1024) * 4)[0]


def seed_bytes(seed_words):
    return struct.pack("<8Q", *[int(w) for w in seed_words])


def fill_blake2xb(words, seed_words, first, bound):
    sb = seed_bytes(seed_words)
    return u64([blake_value(sb, first + i) % bound for i in range(words)])


BLAKE_FIRST = [0, 1, 15, 16, 17, 1023, (1 << 32) + 5]
BLAKE_WORDS = [1, 2, 15, 16, 17, 1025]


# ------------------------------------------------------------------------------------------------------------- the slots
def scatter_slots(vals, mp):
    """out[b][map[i]] = in[b][i]"""
    out = np.zeros_like(vals)
    out[:, np.asarray(mp, dtype=np.int64)] = vals
    return out


def gather_slots(vals, mp):
    """out[b][i] = in[b][map[i]]"""
    return vals[:, np.asarray(mp, dtype=np.int64)]


def rotation(n):
    """a permutation that is not its own inverse: i -> i + 5 mod n"""
    return (np.arange(n) + 5) % n


# ------------------------------------------------------------------------------------------------------------- ALGEBRAIZE
ALGEBRAIZE_PARAMS = [(4, 32, 128), (8, 16, 128), (2, 64, 128), (7, 20, 128), (4, 20, 80), (5, 20, 80), (3, 61, 128), (1, 61, 40)]


def item_int(words):
    return int(words[0]) | int(words[1]) << 64


def felt(item, j, bpf, item_bits):
    """bits [j bpf, j bpf + bpf) of the item's first item_bits bits"""
    take = max(0, min(bpf, item_bits - j * bpf))
    return ((item & ((1 << item_bits) - 1)) >> (j * bpf)) & ((1 << take) - 1)


def algebraize(items, felts, bpf, item_bits):
    return u64([felt(item_int(w), j, bpf, item_bits) for w in items for j in range(felts)])


def algebraize_items(count, rng):
    """all 0xFF, all 0, the walking one, random -- `count` items [count][2]"""
    rows = [[M64, M64], [0, 0]] + [[(1 << b) & M64, (1 << b) >> 64] for b in range(128)]
    rows += rng.integers(0, 1 << 63, (max(0, count - len(rows)), 2), dtype=np.uint64).tolist()
    return u64(rows[:count])


def algebraize_counts(felts):
    """counts whose count * felts lies at and around 256, the workgroup's lanes: 255, 256, 257 where felts divides them"""
    return sorted({c for t in (255, 256, 257) for c in (t // felts, -(-t // felts)) if c >= 1})


# ------------------------------------------------------------------------------------------------------------- PACK_BLOCKS
def pack_block(values, felts, ln):
    """vec_to_oc_block as k_pack_blocks' comment states it: the odd felt's upper half is shifted by len / 2 - 1; 64-bit shifts wrap"""
    mask = (1 << ln) - 1
    mask_lower = (1 << (ln >> 1)) - 1
    mask_higher = mask - mask_lower
    lower = higher = 0
    if felts & 1:
        lower = values[felts - 1] & mask_lower
        higher = (values[felts - 1] & mask_higher) >> ((ln >> 1) - 1)
    for p in range(0, felts - 1, 2):
        lower = ((values[p] & mask) | (lower << ln)) & M64
        higher = ((values[p + 1] & mask) | (higher << ln)) & M64
    return lower, higher


def pack_blocks(vals, n, items, felts, ln):
    """vals [batch][n] -> [batch][items][2]"""
    v = obj(vals).reshape(-1, n)
    return u64([[pack_block([int(x) for x in row[it * felts:it * felts + felts]], felts, ln) for it in range(items)] for row in v])


PACK_FELTS = [1, 2, 3, 4, 7, 8]
PACK_LENS = [2, 17, 20, 32, 61]
