"""GPU tier: a whole resident database from its entries in one call (apsu_he_db_build_from_entries; apsu_amd/csrc/bulk_place.h).
(i) k_entries_scatter alone through the ENTRIES_SCATTER step, against the Python model of tests/test_bulk_place_cpu.py, with a sentinel
in every word nobody may write; (ii) build_database against the incremental path: apply_entries from no BinBundle per bundle index --
same BinBundles, same images byte for byte; (iii) a doubled entry, a device pointer, one shipped parameter set end to end with lookup and
the self-test; (iv) the multi-device handle; (v) the refusals.  All comparisons are exact."""
import numpy as np
import pytest
import torch

import apsu_amd
import common
import test_multi_place_cpu as P
from test_bulk_place_cpu import felt, model_loop

pytestmark = pytest.mark.gpu

SENTINEL = 0xEEEEEEEEEEEEEEEE
ENTRY_INSERTED = apsu_amd.engine.ENTRY_INSERTED


def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)


def kstart_of(counts, ipb, cap):
    """K_l: the running largest ceil(c / cap) of the locations before l in its bundle index"""
    out = []
    for l in range(len(counts)):
        lo = l - l % ipb
        out.append(max([0] + [-(-c // cap) for c in counts[lo:l]]))
    return out


def rand_entries(rng, count):
    """distinct 16-byte items whose first 80 bits are distinct too"""
    e = rng.integers(0, 256, (count, 16), dtype=np.uint8)
    e[:, :4] = np.arange(count, dtype=np.uint32).view(np.uint8).reshape(count, 4)
    return e


def as_int(entry):
    return int.from_bytes(bytes(entry), "little")


def model_bins(G, entries, counts):
    """{(bundle index, k): bins [ipb * F] as lists of felts} by the reference's loop"""
    ipb, F, bpf = int(G.info.items_per_bundle), G.felts_per_item, G.t.bit_length() - 1
    offsets = offsets_of(counts)
    bundles, _ = model_loop(counts, ipb, G.max_items_per_bin)
    out = {}
    for b, per_index in enumerate(bundles):
        for k, locs in enumerate(per_index):
            bins = [[] for _ in range(ipb * F)]
            for loc, here in enumerate(locs):
                for i in here:
                    it = as_int(entries[int(offsets[b * ipb + loc]) + i])
                    for j in range(F):
                        bins[loc * F + j].append(felt(it, j, bpf, bpf * F))
            out[(b, k)] = bins
    return out


def context(**kw):
    return apsu_amd.HeContext(common.toy_json(**kw))


def images(G, bundles):
    return [((b.bundle_idx, b.cache_idx, b.degree), G.save_bundle(b).tobytes()) for b in bundles]


def incremental(G, entries, offsets):
    """the parent's path: apply_entries from no BinBundle, bundle index by bundle index -> the appended Bundles in that order"""
    out = []
    felts = G.algebraize_items(entries)
    for b, (lo, hi, start) in enumerate(G.bucket_entries(offsets)):
        if hi > lo:
            res = G.apply_entries([], inserts=(felts[lo:hi], start), bundle_idx=b)
            assert (res.ins_status == ENTRY_INSERTED).all()
            out += res.appended
    return out


# ------------------------------------------------------------------------------------------------------------- the kernel alone
# toy: n = 64, F = 5, 12 locations per bundle index, 60 of 64 slots used, cap = 10.  One list over two bundle indices: an empty location
# between full ones; later locations with fewer entries than K cap (newest BinBundles first); a location that fills every BinBundle and
# opens two more; the first location of the second index, where K restarts at 0
EDGE_COUNTS = [10, 0, 10, 20, 0, 5, 40, 3, 0, 11, 9, 31,
               25, 7, 0, 30, 1, 10, 50, 0, 49, 41, 2, 50]


@pytest.mark.parametrize("plain_bits, bpf", [(17, 16), (21, 20)])      # felt 4 starts at bit 64; felt 3 crosses it
def test_scatter_kernel_alone(plain_bits, bpf):
    G = context(plain_bits=plain_bits)
    n, F, ipb, cap = G.n, G.felts_per_item, int(G.info.items_per_bundle), 10
    assert (n, F, ipb, G.t.bit_length() - 1, G.bundle_idx_count) == (64, 5, 12, bpf, 2)
    rng = np.random.default_rng(plain_bits)
    counts = EDGE_COUNTS
    offsets, kstart = offsets_of(counts), kstart_of(counts, ipb, cap)
    assert kstart[ipb] == 0 and kstart[6] == 2 and kstart[7] == 4
    entries = rng.integers(0, 256, (int(offsets[-1]), 16), dtype=np.uint8)
    entries[:3] = [[0] * 16, [255] * 16, [0] * 7 + [128, 1] + [0] * 7]
    bundles, _ = model_loop(counts, ipb, cap + 1)
    assert [len(x) for x in bundles] == [4, 5]
    for b in range(2):
        lo = b * ipb
        words = np.ascontiguousarray(entries[int(offsets[lo]):int(offsets[lo + ipb])]).view(np.uint64).reshape(-1, 2)
        off_b = np.ascontiguousarray(offsets[lo:lo + ipb + 1])
        ks_b = np.array(kstart[lo:lo + ipb], dtype=np.uint64)
        for k in range(len(bundles[b])):
            stride = max(len(x) for x in bundles[b][k])
            roots = np.full((n, stride), SENTINEL, dtype=np.uint64)          # bins = n: the root lists of slots 60 .. 63 stay untouched too
            cnt = np.full(n, SENTINEL, dtype=np.uint64)
            G.debug_run_step("entries_scatter", 0, [words, off_b, ks_b], [roots, cnt], batch=ipb, polys=F, terms=stride, e0=k)
            want, want_cnt = np.full((n, stride), SENTINEL, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
            for loc in range(ipb):
                here = bundles[b][k][loc]
                want_cnt[loc * F:loc * F + F] = len(here)
                for r, i in enumerate(here):
                    it = as_int(entries[int(offsets[lo + loc]) + i])
                    for j in range(F):
                        want[loc * F + j, r] = felt(it, j, bpf, bpf * F)
            assert (cnt == want_cnt).all(), (b, k)
            assert (roots == want).all(), (b, k)
    # refused, nothing launched: a chunk longer than stride, offsets that decrease
    words = np.ascontiguousarray(entries[:int(offsets[ipb])]).view(np.uint64).reshape(-1, 2)
    args = dict(batch=ipb, polys=F, e0=0)
    with pytest.raises(ValueError, match="longer than stride"):
        G.debug_run_step("entries_scatter", 0, [words, np.ascontiguousarray(offsets[:ipb + 1]), np.array(kstart[:ipb], dtype=np.uint64)],
                         [np.zeros((n, 9), dtype=np.uint64), np.zeros(n, dtype=np.uint64)], terms=9, **args)
    bad = offsets[:ipb + 1].copy()
    bad[3], bad[4] = bad[4], bad[3]
    with pytest.raises(ValueError, match="offsets decrease"):
        G.debug_run_step("entries_scatter", 0, [words, bad, np.array(kstart[:ipb], dtype=np.uint64)],
                         [np.zeros((n, 10), dtype=np.uint64), np.zeros(n, dtype=np.uint64)], terms=10, **args)
    G.close()


# ------------------------------------------------------------------------------------------------------------- against the parent's path
def spread_counts(rng, T, most):
    """per-location counts with the largest equal to `most`, empty locations among them"""
    counts = [int(v) for v in rng.integers(0, most + 1, T)]
    i, j = (int(v) for v in rng.choice(T, 2, replace=False))
    counts[i], counts[j] = most, 0
    return counts


def index_counts(rng, G, most):
    """spread_counts per bundle index: every bundle index reaches `most`"""
    ipb = int(G.info.items_per_bundle)
    return [c for _ in range(G.bundle_idx_count) for c in spread_counts(rng, ipb, most)]


@pytest.mark.parametrize("table_mult", [1, 2])
@pytest.mark.parametrize("most, per_index", [(10, 1), (20, 2), (38, 4)])        # cap = 10
def test_build_database_equals_apply_entries_from_empty(table_mult, most, per_index):
    G = context(table_mult=table_mult)
    rng = np.random.default_rng(100 * table_mult + most)
    assert G.bundle_idx_count == table_mult
    offsets = offsets_of(index_counts(rng, G, most))
    entries = rand_entries(rng, int(offsets[-1]))
    assert G.entries_plan(offsets).tolist() == [per_index] * G.bundle_idx_count
    got = G.build_database(entries, offsets)
    want = incremental(G, entries, offsets)
    assert [(b.bundle_idx, b.cache_idx) for b in got] == [(b, k) for b in range(G.bundle_idx_count) for k in range(per_index)]
    assert [k for k, _ in images(G, got)] == [k for k, _ in images(G, want)]
    for (key, a), (_, w) in zip(images(G, got), images(G, want)):
        assert a == w, key
    copy_ms, scatter_ms, build_ms = G.build_times()
    assert copy_ms > 0 and scatter_ms > 0 and build_ms > 0
    G.close()


def test_a_bundle_index_without_entries_gets_no_bundle():
    G = context()
    ipb = int(G.info.items_per_bundle)
    counts = [0] * ipb + [3] * ipb
    offsets = offsets_of(counts)
    entries = rand_entries(np.random.default_rng(5), int(offsets[-1]))
    assert G.entries_plan(offsets).tolist() == [0, 1]
    got = G.build_database(entries, offsets)
    assert [(b.bundle_idx, b.cache_idx, b.degree) for b in got] == [(1, 0, 3)]
    assert [i for _, i in images(G, got)] == [i for _, i in images(G, incremental(G, entries, offsets))]
    assert G.build_database(np.zeros((0, 16), dtype=np.uint8), offsets_of([0] * (2 * ipb))) == []
    G.close()


def test_a_doubled_entry_is_a_double_root():
    G = context()
    ipb = int(G.info.items_per_bundle)
    rng = np.random.default_rng(11)
    counts = [4, 12, 0, 7] + [2] * (2 * ipb - 4)
    offsets = offsets_of(counts)
    entries = rand_entries(rng, int(offsets[-1]))
    entries[int(offsets[1]) + 3] = entries[int(offsets[1]) + 1]            # twice in location 1, both in BinBundle 0
    entries[int(offsets[3]) + 6] = entries[int(offsets[3])]
    got = G.build_database(entries, offsets)
    model = model_bins(G, entries, counts)
    assert [(b.bundle_idx, b.cache_idx) for b in got] == sorted(model)
    doubled = model[(0, 0)][5]
    assert len(doubled) == 10 and len(set(doubled)) == 9
    for b in got:
        want = G.build_bundle(b.bundle_idx, b.cache_idx, model[(b.bundle_idx, b.cache_idx)])
        assert b.degree == want.degree and G.save_bundle(b).tobytes() == G.save_bundle(want).tobytes()
    G.close()


def test_entries_on_the_device_give_the_same_images():
    G = context()
    rng = np.random.default_rng(13)
    offsets = offsets_of(index_counts(rng, G, 25))
    entries = rand_entries(rng, int(offsets[-1]))
    host = images(G, G.build_database(entries, offsets))
    for shift in (0, 8):                                                   # a device pointer that is 16-byte aligned, and one that is not
        buf = torch.zeros(entries.size + 16, dtype=torch.uint8, device="cuda")
        buf[shift:shift + entries.size] = torch.from_numpy(entries.reshape(-1)).cuda()
        torch.cuda.synchronize()                                           # (the engine's stream does not wait for torch's)
        assert images(G, G.build_database(buf.data_ptr() + shift, offsets)) == host
    for blocks in (1, 3):                                                  # the grid is a matter of speed alone (cap = 10: one block holds a chunk)
        G.set_scatter_blocks(blocks)
        assert images(G, G.build_database(entries, offsets)) == host
    G.close()


def test_shipped_set_end_to_end():
    """256K-512, 300 items: bucket_items -> identity OPRF -> build_database; every item is then present, and a real query over the
    result agrees with the plaintext answer in every slot"""
    G = apsu_amd.HeContext(common.param_json("256K-512"))
    rng = np.random.default_rng(0x32353651)
    db = rng.integers(0, 256, (300, 16), dtype=np.uint8)
    offsets, order = G.bucket_items(db)
    entries = db[order]
    bundles = G.build_database(entries, offsets)
    assert len(bundles) == int(G.entries_plan(offsets).sum()) >= 1
    (lo, hi, start), = G.bucket_entries(offsets)
    present, _ = G.lookup(bundles, (G.algebraize_items(entries), start))
    assert present.shape == (len(bundles), len(order)) and present.any(axis=0).all()
    rep = G.self_test(bundles)
    assert rep.bundles == len(bundles) and rep.mismatches == 0 and rep.first_mismatch is None
    G.close()


# ------------------------------------------------------------------------------------------------------------- the handle
def handle_state(G, M, tmp_path, tag):
    path = str(tmp_path / ("db_%s.bin" % tag))
    M.save_db_file(path)
    reg = [tuple(M.bundle_info(i)) for i in range(M.bundle_count())]
    return reg, [((b.bundle_idx, b.cache_idx, b.degree), G.save_bundle(b).tobytes()) for b in G.load_db_file(path)]


def test_handle_builds_the_same_database(tmp_path):
    js = common.toy_json()
    G = apsu_amd.HeContext(js)
    M = apsu_amd.MultiContext(js, [0, 0, 0])
    ipb, nidx, world = int(G.info.items_per_bundle), G.bundle_idx_count, 3
    rng = np.random.default_rng(17)
    # first the entries of bundle index 1 alone, then those of index 0: the second call appends behind the first
    c1 = [0] * ipb + spread_counts(rng, ipb, 33)
    c0 = spread_counts(rng, ipb, 18) + [0] * ipb
    load, want_reg, want_img = [0] * world, [], []
    for tag, counts in (("one", c1), ("zero", c0)):
        offsets = offsets_of(counts)
        entries = rand_entries(rng, int(offsets[-1]))
        single = G.build_database(entries, offsets)
        before = M.bundle_count()
        ids = M.build_database(entries, offsets)
        assert ids == list(range(before, before + len(single))) and M.bundle_count() == before + len(single)     # dense
        for b in single:                                                   # the placement rule, loads taken as each one registers
            cand = P.candidates(b.bundle_idx, nidx, world)
            slot = min(cand, key=lambda s: (load[s], s))
            load[slot] += b.degree + 64
            want_reg.append((slot, b.bundle_idx, b.cache_idx, b.degree))
        want_img += images(G, single)
        reg, img = handle_state(G, M, tmp_path, tag)
        assert reg == want_reg
        assert img == want_img
    assert len({r[0] for r in want_reg}) >= 2                              # (more than one slot took part)
    # refused: bundle index 0 holds BinBundles now; the handle stays as it is
    offsets = offsets_of([2] * ipb + [0] * ipb)
    with pytest.raises(ValueError, match="holds a BinBundle already"):
        M.build_database(rand_entries(rng, int(offsets[-1])), offsets)
    assert handle_state(G, M, tmp_path, "after") == (want_reg, want_img)
    M.close()
    G.close()


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_context_working():
    G = context()
    rng = np.random.default_rng(19)
    offsets = offsets_of(index_counts(rng, G, 25))
    entries = rand_entries(rng, int(offsets[-1]))
    total = int(G.entries_plan(offsets).sum())
    assert total == 6
    with pytest.raises(ValueError, match="6 BinBundles come out.*room for 5"):
        G.build_database(entries, offsets, count=5)
    bad = offsets.copy()
    bad[2], bad[3] = max(bad[2], bad[3]) + 1, min(bad[2], bad[3])
    with pytest.raises(ValueError, match="offsets decrease at location 2"):
        G.build_database(entries, bad)
    with pytest.raises(ValueError, match="offsets decrease"):
        G.entries_plan(bad)
    with pytest.raises(ValueError, match="entries"):
        G.build_database(entries[:-1], offsets)
    want = images(G, incremental(G, entries, offsets))
    assert images(G, G.build_database(entries, offsets)) == want            # the context goes on working
    G.close()
    # max_items_per_bin = 1: no entry fits below max_items_per_bin - 1 = 0 items
    G1 = context(max_items=1, ps_low=0, query_powers=(1,))
    off1 = offsets_of([1] * G1.table_size)
    with pytest.raises(ValueError, match="max_items_per_bin = 1"):
        G1.build_database(rand_entries(rng, int(off1[-1])), off1)
    with pytest.raises(ValueError, match="max_items_per_bin = 1"):
        G1.entries_plan(off1)
    b = G1.build_bundle(0, 0, [[3], [], [5]])                              # the context goes on working
    assert b.degree == 1
    G1.close()
