"""N5, the querier's side, CPU tier: the device functions of apsu_amd/csrc/query_side.h (the code k_sample_ternary, k_sample_cbd and
k_plain_powers run) through libapsu_he_hostemu.so against a Python restatement of the header's documented streams."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common  # noqa: E402
import emu_lib  # noqa: E402
import query_side_model as M  # noqa: E402

u64p = C.POINTER(C.c_uint64)
SEEDS = [bytes(range(64)), bytes((7 * i + 201) & 0xFF for i in range(64))]
RINGS = [64, 4096, 8192]


@pytest.fixture(scope="module")
def emu():
    lib = emu_lib.load()
    lib.emu_qs_block.argtypes = [C.c_int, C.c_uint64, C.c_uint64]
    return lib


def _p(a):
    return a.ctypes.data_as(u64p)


@pytest.mark.parametrize("n", RINGS)
@pytest.mark.parametrize("seed", SEEDS)
def test_secret_stream_matches_model(emu, seed, n):
    sd = M.seed_words(seed)
    out = np.zeros(n, dtype=np.int8)
    assert emu.emu_qs_secret(_p(sd), C.c_uint64(n), C.c_void_p(out.ctypes.data)) == 0
    exp = M.secret(seed, n)
    assert set(np.unique(exp)) <= {-1, 0, 1}
    assert (out.astype(np.int64) == exp).all()


@pytest.mark.parametrize("n", RINGS)
@pytest.mark.parametrize("seed", SEEDS)
def test_noise_stream_matches_model(emu, seed, n):
    sd = M.seed_words(seed)
    for obj in (0, 3, M.KEY_OBJECTS, M.KEY_OBJECTS + 23):
        out = np.zeros(n, dtype=np.int8)
        assert emu.emu_qs_noise(_p(sd), C.c_uint64(obj), C.c_uint64(n), C.c_void_p(out.ctypes.data)) == 0
        exp = M.noise(seed, obj, n)
        assert np.abs(exp).max() <= 21
        assert (out.astype(np.int64) == exp).all(), obj


@pytest.mark.parametrize("seed", SEEDS)
def test_public_seeds_match_model(emu, seed):
    sd = M.seed_words(seed)
    seen = set()
    for obj in (0, 1, 15, 16, 17, 16 + 65534, M.MAX_OBJECTS - 1):
        out = np.zeros(8, dtype=np.uint64)
        assert emu.emu_qs_public_seed(_p(sd), C.c_uint64(obj), _p(out)) == 0
        assert (out == M.public_seed(seed, obj)).all(), obj
        seen.add(out.tobytes())
    assert len(seen) == 7


def test_value_maps():
    # the ternary map splits the 64-bit range into three equal parts (up to one word), the noise map is a difference of two 21-bit counts
    assert M.ternary(0) == -1 and M.ternary((1 << 64) - 1) == 1 and M.ternary(1 << 63) == 0
    thirds = [-(-(k << 64) // 3) for k in (1, 2)]          # first word of the second and third part
    assert M.ternary(thirds[0] - 1) == -1 and M.ternary(thirds[0]) == 0 and M.ternary(thirds[1] - 1) == 0 and M.ternary(thirds[1]) == 1
    sizes = [thirds[0], thirds[1] - thirds[0], (1 << 64) - thirds[1]]
    assert max(sizes) - min(sizes) <= 1                     # bias <= 2^-64 < 2^-60
    assert M.cbd((1 << 21) - 1) == 21 and M.cbd(((1 << 21) - 1) << 21) == -21 and M.cbd((1 << 42) - 1) == 0 and M.cbd(~0 << 42 & (2**64 - 1)) == 0


def test_stream_ranges_are_disjoint(emu):
    lay = np.zeros(8, dtype=np.uint64)
    assert emu.emu_qs_layout(_p(lay), 8) == 7
    max_n, poly_blocks, key_objects, max_objects, secret0, seed0, noise0 = (int(v) for v in lay[:7])
    # the constants the kernels use are the ones the header (and the Python model) state
    assert (max_n, poly_blocks, key_objects, max_objects, secret0, seed0, noise0) == (
        M.MAX_N, M.POLY_BLOCKS, M.KEY_OBJECTS, M.MAX_OBJECTS, M.SECRET_BLOCK0, M.SEED_BLOCK0, M.NOISE_BLOCK0)
    assert poly_blocks * 8 >= max_n                         # one word per coefficient of the largest ring
    ranges = [(secret0, secret0 + poly_blocks), (seed0, seed0 + max_objects), (noise0, noise0 + max_objects * poly_blocks)]
    ranges.sort()
    for (a0, a1), (b0, b1) in zip(ranges, ranges[1:]):
        assert a0 < a1 <= b0 < b1
    assert ranges[-1][1] * 64 < 1 << 64                     # byte positions fit the generator's 64-bit buffer counter many times over
    # per object: noise ranges of neighbouring objects do not touch, and the block functions stay inside their ranges at the extremes
    blk = emu.emu_qs_block
    assert blk(0, 0, 0) == secret0 and blk(0, 0, max_n - 1) == secret0 + poly_blocks - 1
    assert blk(1, 0, 0) == seed0 and blk(1, max_objects - 1, 0) == seed0 + max_objects - 1
    for o in (0, 1, key_objects - 1, key_objects, max_objects - 2):
        assert blk(2, o, max_n - 1) + 1 == blk(2, o + 1, 0) == noise0 + (o + 1) * poly_blocks
    assert key_objects >= 8                                 # K - 1 <= 8 relinearisation keys


PARAM_SETS = [("toy", common.toy_json()), ("1M-1024-com", common.param_json("1M-1024-com")),
              ("16M-4096", common.param_json("16M-4096")), ("256M-4096", common.param_json("256M-4096"))]


@pytest.mark.parametrize("name,js", PARAM_SETS, ids=[p[0] for p in PARAM_SETS])
def test_plain_powers_match_pow(emu, name, js):
    info = np.zeros(64, dtype=np.uint64)
    assert emu.emu_params_info(js.encode(), _p(info), 64) > 0
    t = int(info[3])
    sources = sorted(int(p) for p in json.loads(js)["query_params"]["query_powers"])
    rng = np.random.default_rng(5)
    xs = [0, 1, 2, t - 1, t - 2, t // 2] + [int(v) for v in rng.integers(0, t, 200)]
    x = np.array([v for v in xs for _ in sources], dtype=np.uint64)
    e = np.array(sources * len(xs), dtype=np.uint32)
    out = np.zeros(x.size, dtype=np.uint64)
    assert emu.emu_qs_pow_mod(C.c_uint64(t), _p(x), C.c_void_p(e.ctypes.data), _p(out), int(x.size)) == 0
    exp = [pow(int(a), int(b), t) for a, b in zip(x, e)]
    assert [int(v) for v in out] == exp
