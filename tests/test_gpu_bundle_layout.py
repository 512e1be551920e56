"""GPU tier: the stored layout of a BinBundle (apsu_amd/csrc/bundle_layout.h) at its edges, on the toy ring (n = 64, h = 4,
max_items_per_bin = 11: the smallest shape with every kind of run) at degrees 0, 1, 3, 4, 5, 7, 8, 11, and without
Paterson-Stockmeyer (ps_low_degree = 0, max_items_per_bin = 6) at degrees 0, 1, 6.

Same bytes as before the layout became one function: the SHA-256 of save_bundle(build_bundle(0, 0, gen_bins(...))) and of
save_bundle(random_bundle(0, 0, degree, 1)) for every case, with bit-packed rows (in this process) and with dense rows
(APSU_HE_PACKED_ROWS=0, one fresh child process), is held to tests/golden/bundle_layout_parent.json.  That file was made at the
parent commit (4173c4e), with this file copied into its tests/ directory, by
    PYTHONPATH=. python tests/test_gpu_bundle_layout.py tests/golden/bundle_layout_parent.json
Decode is the inverse of encode: an update with nothing to insert or remove (decode_bundle, then the tail of the build) reproduces
the image, and bin_counts gives back the generator's counts.  Where a coefficient is: bundle_coeff's kind against the rule restated
here (bin_bundle.cpp:385-420)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import apsu_amd
import common
from oracle import ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "bundle_layout_parent.json")
SHAPES = {
    "ps3": (dict(), (0, 1, 3, 4, 5, 7, 8, 11)),
    "ps0": (dict(ps_low=0, max_items=6, query_powers=(1, 2, 3, 5)), (0, 1, 6)),
}
CASES = [(key, d) for key in sorted(SHAPES) for d in SHAPES[key][1]]
N_BINS = 60


def gen_bins(t, degree):
    """60 bins of the 64 slots: bin 5 holds `degree` items, bin 3 none, bin s (7 s + degree) mod (degree + 1); the values come from a
    64-bit linear congruential generator seeded by the degree, non-zero and distinct within a bin"""
    state = [0x9E3779B97F4A7C15 ^ degree]

    def value():
        state[0] = (state[0] * 6364136223846793005 + 1442695040888963407) % 2 ** 64
        return (state[0] >> 33) % (t - 1) + 1

    bins = []
    for s in range(N_BINS):
        count = degree if s == 5 else 0 if s == 3 else (7 * s + degree) % (degree + 1)
        b = []
        while len(b) < count:
            v = value()
            if v not in b:
                b.append(v)
        bins.append(b)
    return bins


def coeff_kind(ps, d):
    """0: a_0, raw mod t; 1: NTT form at the plaintexts' level; 2: coefficient form (stored pre-lifted at the high level)"""
    if d == 0:
        return 0
    return 1 if (not ps and d != 0) or (ps and d % (ps + 1) != 0) else 2


def sha(G, b):
    return hashlib.sha256(G.save_bundle(b).tobytes()).hexdigest()


class World:
    """one context per shape, and per case the generator's bins, their BinBundle and the random BinBundle"""

    def __init__(self):
        self.G, self.ps, self.bins, self.built, self.random = {}, {}, {}, {}, {}
        for key, (kw, degrees) in SHAPES.items():
            js = common.toy_json(**kw)
            p = ref.load_params(js)
            t = ref.RefContext.from_params(p).t
            G = self.G[key] = apsu_amd.HeContext(js)
            self.ps[key] = p["ps_low_degree"]
            for d in degrees:
                self.bins[key, d] = gen_bins(t, d)
                self.built[key, d] = G.build_bundle(0, 0, self.bins[key, d])
                self.random[key, d] = G.random_bundle(0, 0, d, 1)
                assert self.built[key, d].degree == d

    def hashes(self):
        """{shape: {degree: {"build": sha256, "random": sha256}}} and the row format of the images (1 bit-packed, 0 dense)"""
        out, formats = {}, set()
        for key, d in CASES:
            out.setdefault(key, {})[str(d)] = {"build": sha(self.G[key], self.built[key, d]), "random": sha(self.G[key], self.random[key, d])}
            formats.add(int(self.G[key].save_bundle(self.built[key, d])[8 + 16 + 88 + 8 + 28:][:4].view(np.uint32)[0]))
        assert len(formats) == 1
        return out, formats.pop()

    def close(self):
        for G in self.G.values():
            G.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import test_gpu_bundle_layout as T
w = T.World()
hashes, row_format = w.hashes()
w.close()
json.dump({"hashes": hashes, "row_format": row_format}, open(sys.argv[3], "w"))
"""


def dense_hashes(path):
    """the same images from a context that keeps dense rows: APSU_HE_PACKED_ROWS is read when a context is created -> a fresh process"""
    env = dict(os.environ, APSU_HE_PACKED_ROWS="0")
    subprocess.run([sys.executable, "-c", CHILD, os.path.dirname(HERE), HERE, path], env=env, check=True, timeout=120)
    with open(path) as f:
        got = json.load(f)
    assert got["row_format"] == 0, "the child kept dense rows"
    return got["hashes"]


def test_packed_images_are_the_parents_bytes(world, golden):
    hashes, row_format = world.hashes()
    assert row_format == 1
    for key, d in CASES:
        print(key, d, hashes[key][str(d)])
    assert hashes == golden["packed"]


def test_dense_images_are_the_parents_bytes(tmp_path, golden):
    assert dense_hashes(str(tmp_path / "dense.json")) == golden["dense"]


@pytest.mark.parametrize("key,d", CASES)
def test_decode_is_the_inverse_of_encode(world, key, d):
    G = world.G[key]
    for b in (world.built[key, d], world.random[key, d]):
        again = G.update_bundle(b)                            # nothing inserted, nothing removed: decode, then the tail of the build
        assert again.degree == d
        assert G.save_bundle(again).tobytes() == G.save_bundle(b).tobytes()
    want = np.full(G.n, apsu_amd.engine.NOT_A_BIN, dtype=np.uint32)
    want[:N_BINS] = [len(b) for b in world.bins[key, d]]
    assert (G.bin_counts(world.built[key, d]) == want).all()


@pytest.mark.parametrize("key,degree", [("ps3", 11), ("ps0", 6)])
def test_where_a_coefficient_is(world, key, degree):
    G = world.G[key]
    for b in (world.built[key, degree], world.random[key, degree]):
        for d in range(degree + 1):
            got, kind = G.bundle_coeff(b, d)
            assert kind == coeff_kind(world.ps[key], d), d
        with pytest.raises(ValueError):
            G.bundle_coeff(b, degree + 1)


if __name__ == "__main__":
    w = World()
    packed, row_format = w.hashes()
    w.close()
    assert row_format == 1
    with open(sys.argv[1], "w") as f:
        json.dump({"packed": packed, "dense": dense_hashes(sys.argv[1] + ".dense")}, f, indent=1, sort_keys=True)
        f.write("\n")
    os.remove(sys.argv[1] + ".dense")
