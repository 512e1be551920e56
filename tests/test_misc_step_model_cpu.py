"""CPU tier: the models of tests/misc_step_model.py (the steps ADD .. PACK_BLOCKS) held to the independent statements the tree already has:
oracle/blake2x.py's generator, the emulation's felt split (emu_query_values: cuckoo_item_felt), BatchEncoder's slot map as the oracle and
the querier's model state it, the oracle's vec_to_oc_block, and splitmix64's published outputs."""
import ctypes as C
import types

import numpy as np
import pytest

import emu_lib
import misc_step_model as M
import query_step_model
from emu_lib import vp
from oracle import blake2x, pymodel
from test_bulk_place_cpu import felt as bulk_felt


def test_splitmix64_reference_outputs():
    """the first outputs of splitmix64 seeded with 0 (Vigna's reference implementation), and the wrap of seed + i gamma"""
    assert [int(x) for x in M.fill_random(3, 0, M.M64)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert int(M.fill_random(1, M.M64, M.M64)[0]) == M.splitmix64(M.GAMMA - 1)
    assert (M.fill_random(300, 12345, 1) == 0).all() and set(M.fill_random(300, 12345, 2).tolist()) == {0, 1}


@pytest.mark.parametrize("first", [0, 1, 15, 16, 17, 1023])
def test_blake2xb_model_equals_the_generator(first):
    seed = np.random.default_rng(first).integers(0, 1 << 63, 8, dtype=np.uint64)
    for words in (1, 2, 17, 1025):                          # first = 1023, words = 2 crosses a 4096-byte buffer
        want = blake2x.Blake2xbPRNG(seed).values(words, skip=first)
        assert M.fill_blake2xb(words, seed, first, 1 << 40).tolist() == want
        assert M.fill_blake2xb(words, seed, first, 65537).tolist() == [v % 65537 for v in want]
    assert (M.fill_blake2xb(5, seed, first, 1) == 0).all()
    assert M.blake_value(M.seed_bytes(seed), (1 << 32) + 5) == M.blake_value(M.seed_bytes(seed), (1 << 32) + 5) < 1 << 32


@pytest.mark.parametrize("felts, bpf, item_bits", M.ALGEBRAIZE_PARAMS)
def test_algebraize_model_equals_the_emulations_felt_split(felts, bpf, item_bits):
    emu = emu_lib.load()
    count = 140
    items = M.algebraize_items(count, np.random.default_rng(felts * bpf))
    got = np.zeros(count * felts, dtype=np.uint64)
    emu.emu_query_values(vp(items), C.c_uint32(1), C.c_uint32(count), C.c_uint32(felts), C.c_uint32(bpf), C.c_uint32(item_bits), C.c_uint64(count * felts), vp(got))
    want = M.algebraize(items, felts, bpf, item_bits)
    assert (got == want).all()
    for w in items[:40]:
        for j in range(felts):
            if j * bpf < item_bits:
                assert M.felt(M.item_int(w), j, bpf, item_bits) == bulk_felt(M.item_int(w), j, bpf, item_bits)
    # every shift branch is there: a felt from bit 0, inside the low word, across bit 64 or from it on, short, empty
    offs = [j * bpf for j in range(felts)]
    assert 0 in offs
    if (felts, bpf, item_bits) == (7, 20, 128):
        assert 60 in offs and 120 in offs and item_bits - 120 < bpf           # across bit 64; a short last felt
    if (felts, bpf, item_bits) == (5, 20, 80):
        assert offs[4] >= item_bits                                            # an empty felt
    if (felts, bpf, item_bits) == (2, 64, 128):
        assert 64 in offs                                                      # a felt that starts on bit 64


@pytest.mark.parametrize("n", [64, 1024, 4096])
def test_slot_models_on_the_contexts_map(n):
    mp = query_step_model.slot_map(n)
    assert mp == pymodel.Model.slot_map(types.SimpleNamespace(n=n, logn=n.bit_length() - 1))      # (the oracle's method reads n and logn alone)
    assert sorted(mp) == list(range(n))
    vals = np.random.default_rng(n).integers(0, 1 << 63, (3, n), dtype=np.uint64)
    for m in (mp, M.rotation(n)):
        s = M.scatter_slots(vals, m)
        assert all(s[b, m[i]] == vals[b, i] for b in range(3) for i in (0, 1, n // 2, n - 1))
        assert (M.gather_slots(s, m) == vals).all()
    rot = M.rotation(n)
    assert (M.scatter_slots(vals, rot) != M.gather_slots(vals, rot)).any()      # not its own inverse: the two kernels differ on it


@pytest.mark.parametrize("ln", M.PACK_LENS)
def test_pack_block_model_equals_the_oracle(ln):
    rng = np.random.default_rng(ln)
    plain_modulus = 1 << (ln - 1)                           # the oracle derives len = ln from it
    for felts in M.PACK_FELTS:
        for vals in ([M.M64] * felts, [0] * felts, [int(x) for x in rng.integers(0, 1 << 63, felts)], [int(x) % plain_modulus for x in rng.integers(0, 1 << 63, felts)]):
            assert M.pack_block(vals, felts, ln) == pymodel.vec_to_oc_block(vals, felts, plain_modulus)


def test_add_clear_and_report_models():
    q, n = [97, 193], 8
    a, b = M.add_operands(q, n, 1, 1, np.random.default_rng(1))
    s = M.add(a, b, q, n)
    assert all(int(s[0, j, k]) == (int(a[0, j, k]) + int(b[0, j, k])) % q[j] for j in range(2) for k in range(n))
    assert (a[0, 0] == 96).any() and (s < np.array(q, dtype=np.uint64).reshape(1, 2, 1)).all()
    assert M.clear_bits([M.M64, 5], 0).tolist() == [M.M64, 5] and M.clear_bits([M.M64, 5], 1).tolist() == [M.M64 - 1, 4]
    assert int(M.clear_bits([M.M64], 63)[0]) == 1 << 63
    src = np.zeros((1, 2, 2, n), dtype=np.uint64)
    assert M.sources_report(src, q, n, 7, 9) == 7
    src[0, 1, 0, 3] = 97                                     # >= its own prime, below the neighbouring limb's
    assert M.sources_report(src, q, n, 7, 9) == 9 and M.sources_report(src, q, n, 10, 9) == 10
    src[0, 1, 0, 3], src[0, 1, 1, 3] = 96, 192
    assert M.sources_report(src, q, n, 7, 9) == 7
