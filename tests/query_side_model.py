"""Python restatement of the querier-side random streams documented in include/apsu_he.h (N5), over the independent
Blake2xb model oracle/blake2x.py.  Shared by the CPU and the GPU tests of that feature."""
import struct

import numpy as np

from oracle.blake2x import Blake2xbPRNG

# the layout as the header states it, in 64-byte stream blocks (16 outputs of 32 bits each)
BLOCK_OUTPUTS = 16
POLY_BLOCKS = 4096           # one 64-bit word per coefficient, n <= 32768
SECRET_BLOCK0 = 0
SEED_BLOCK0 = 4096
NOISE_BLOCK0 = 1 << 21
KEY_OBJECTS = 16             # object i = relinearisation key i; object 16 + c = ciphertext c of a query
MAX_OBJECTS = 1 << 20
MAX_N = 32768


def seed_words(seed_bytes):
    return np.frombuffer(bytes(seed_bytes), dtype="<u8").astype(np.uint64)


def outputs(seed, first, count):
    """u[first .. first + count) of the generator under the 64-byte seed, through Blake2xbPRNG(seed).values(...)"""
    per_buffer = Blake2xbPRNG.BUFFER // 4
    g = Blake2xbPRNG(seed)
    g.counter = first // per_buffer                      # buffers are independent: start at the one that holds u[first]
    return g.values(count, skip=first % per_buffer)


def words(seed, block0, count):
    """`count` 64-bit draws w = u[p] + 2^32 u[p + 1] from the first word of stream block block0 on"""
    u = outputs(seed, block0 * BLOCK_OUTPUTS, 2 * count)
    return [u[2 * i] | (u[2 * i + 1] << 32) for i in range(count)]


def ternary(w):
    return ((3 * w) >> 64) - 1


def cbd(w):
    return bin(w & 0x1FFFFF).count("1") - bin((w >> 21) & 0x1FFFFF).count("1")


def secret(seed, n):
    return np.array([ternary(w) for w in words(seed, SECRET_BLOCK0, n)], dtype=np.int64)


def noise(seed, obj, n):
    return np.array([cbd(w) for w in words(seed, NOISE_BLOCK0 + obj * POLY_BLOCKS, n)], dtype=np.int64)


def public_seed(seed, obj):
    return np.array(words(seed, SEED_BLOCK0 + obj, 8), dtype=np.uint64)


def centred(a, q):
    """residues mod q -> signed representatives in (-q/2, q/2] as Python ints"""
    a = a.astype(object)
    return np.where(a > q // 2, a - q, a)
