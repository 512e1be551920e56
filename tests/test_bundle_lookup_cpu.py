"""CPU tier of find-and-place: (i) k_bins_lookup / k_bin_counts as the waves run them (apsu_amd/csrc/bin_lookup.h: lane = slot, the
points grouped by slot through lookup_plan's work list, R accumulators per lane, rows from the top) stepped lane by lane by the CPU
emulation library (emu_bins_lookup, emu_bin_counts) and held to plain Python Horner over bins kept as lists; (ii) the placement rule
(apsu_amd/csrc/db_place.h through emu_place_entries) held to a Python restatement of the reference's loops
(ReceiverDB::remove / insert_or_assign, receiver_db.cpp:349-434,524-567).  All comparisons are exact integers."""
import ctypes as C

import numpy as np
import pytest

import emu_lib
from emu_lib import vp
from test_bundle_update_cpu import T, poly_from_roots

u64p = C.POINTER(C.c_uint64)
NONE = 0xFFFFFFFF
R = 8                                                     # device.h: LOOKUP_R
INSERTED, DUPLICATE, REMOVED, NOT_FOUND = 0, 1, 2, 3
UNCHANGED, REPLACED, EMPTY = 0, 1, 2


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


# ---------------------------------------------------------------------------------------------------------------- lookup
def poly_array(bins, n, rows=None):
    """bins: per slot a list of roots, a coefficient list wrapped as ("poly", [..]), or None (the zero polynomial) -> [rows][n]"""
    polys = []
    for b in bins:
        if b is None:
            polys.append([0])
        elif isinstance(b, tuple):
            polys.append(list(b[1]))
        else:
            polys.append(poly_from_roots(b))
    rows = rows or max(len(p) for p in polys)
    A = np.zeros((rows, n), dtype=np.uint64)
    for s, p in enumerate(polys):
        A[:len(p), s] = p
    return A


def horner(col, x):
    acc = 0
    for c in reversed(col):
        acc = (acc * x + int(c)) % T
    return acc


def model_flags(A, felts, start):
    out = []
    for f, s in zip(felts, start):
        for j, x in enumerate(f):
            col = [int(v) for v in A[:, s + j]]
            out.append(int(any(col) and horner(col, int(x)) == 0))
    return out


def run_lookup(emu, A, felts, start, r=R):
    n = A.shape[1]
    felts = np.ascontiguousarray(felts, dtype=np.uint64).reshape(len(start), -1)
    F = felts.shape[1]
    start = np.ascontiguousarray(start, dtype=np.uint32)
    flags = np.full(len(start) * F, 0xEE, dtype=np.uint8)
    stats = np.zeros(3, dtype=np.uint64)
    A = np.ascontiguousarray(A)
    rc = emu.emu_bins_lookup(C.c_uint64(T), vp(A), C.c_uint64(n), C.c_uint32(A.shape[0] - 1), vp(felts), vp(start), C.c_uint64(len(start)),
                             C.c_uint32(F), C.c_int(r), vp(flags), vp(stats))
    assert rc == 0, emu.emu_last_error()
    return [int(v) for v in flags], [int(v) for v in stats]


def run_counts(emu, A):
    A = np.ascontiguousarray(A)
    counts = np.zeros(A.shape[1], dtype=np.uint32)
    emu.emu_bin_counts(vp(A), C.c_uint64(A.shape[1]), C.c_uint32(A.shape[0]), vp(counts))
    return [int(v) for v in counts]


def mixed_points(rng, bins, per_slot=2):
    """single-part entries: for every slot a root of it (if it has one) and values drawn at random"""
    felts, start = [], []
    for s, b in enumerate(bins):
        roots = b if isinstance(b, list) else []
        for k in range(per_slot):
            felts.append([roots[int(rng.integers(0, len(roots)))] if roots and k == 0 else int(rng.integers(0, T))])
            start.append(s)
    return felts, start


@pytest.mark.parametrize("degree", [0, 1, 63, 64, 65, 200])
def test_lookup_against_python_horner(emu, degree):
    """ragged bins up to `degree` in two tiles (n = 128), every slot asked for one of its roots and a random value; the rows are
    taken four at a time, so the degrees around 64 and the small ones cover every remainder of the row loop"""
    rng = np.random.default_rng(200 + degree)
    n = 128
    bins = [[int(v) for v in rng.integers(0, T, degree if s % 3 == 0 else int(rng.integers(0, degree + 1)))] for s in range(n)]
    A = poly_array(bins, n)
    assert A.shape[0] == degree + 1
    felts, start = mixed_points(rng, bins)
    got, stats = run_lookup(emu, A, felts, start)
    want = model_flags(A, felts, start)
    assert got == want
    assert degree == 0 or (0 < sum(want) < len(want))     # both answers occur
    assert run_counts(emu, A) == [len(b) for b in bins]
    # felts_per_item = 3: parts of one entry in consecutive slots, the AND left to the caller
    felts3 = [[int(rng.integers(0, T)) if rng.random() < 0.3 or not bins[s + j] else bins[s + j][0] for j in range(3)] for s in range(0, n - 3, 2)]
    start3 = list(range(0, n - 3, 2))
    assert run_lookup(emu, A, felts3, start3)[0] == model_flags(A, felts3, start3)


def test_zero_point_double_root_one_and_the_zero_polynomial(emu):
    n = 64
    bins = [[0, 5, 9], [5, 9], [7, 7, 3], [], None, ("poly", [0, 0, 1]), ("poly", [3]), ("poly", [0, 4])] + [None] * (n - 8)
    A = poly_array(bins, n)
    felts = [[0], [0], [7], [3], [0], [1], [0], [123], [0], [1], [0], [0], [5]]
    start = [0, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 7]
    got, _ = run_lookup(emu, A, felts, start)
    want = model_flags(A, felts, start)
    assert got == want
    #        x=0 root  x=0 none  double  single  "1" at 0  "1" at 1  zero polynomial (Horner gives 0)  x^2 at 0  x^2 at 1  3   4x at 0  4x at 5
    assert want == [1, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 1, 0]
    counts = run_counts(emu, A)
    assert counts[:8] == [3, 2, 3, 0, NONE, 2, 0, 1] and all(c == NONE for c in counts[8:])
    # nothing is ever found in a slot without a polynomial, whatever the point, also next to slots that are bins
    felts = [[int(v)] for v in range(40)]
    assert run_lookup(emu, A, felts, [4] * 40)[0] == [0] * 40
    assert run_lookup(emu, A, [[5, 9, 7, 0, 0]], [0])[0] == [1, 1, 1, 0, 0]


def test_one_slot_holds_three_chunks_and_one_point(emu):
    """a tile whose points all sit in one slot: 3R + 1 rows of 64 words for 3R + 1 parts, four work items, the last of one row"""
    rng = np.random.default_rng(5)
    n = 192
    bins = [[int(v) for v in rng.integers(0, T, 20)] for _ in range(n)]
    A = poly_array(bins, n)
    slot = 64 + 17
    pts = [bins[slot][k % 20] if k % 2 else int(rng.integers(0, T)) for k in range(3 * R + 1)]
    got, stats = run_lookup(emu, A, [[p] for p in pts], [slot] * len(pts))
    assert got == model_flags(A, [[p] for p in pts], [slot] * len(pts)) and 0 < sum(got) < len(got)
    assert stats == [4, 3 * R + 1, R]                      # work items, rows, widest work item
    # every entry at the same start bin (felts_per_item = 5): the storage stays one row per entry
    felts = [[bins[10 + j][k % 20] if (k + j) % 3 else int(rng.integers(0, T)) for j in range(5)] for k in range(50)]
    got, stats = run_lookup(emu, A, felts, [10] * 50)
    assert got == model_flags(A, felts, [10] * 50)
    assert stats[:2] == [(50 + R - 1) // R, 50]


def test_points_in_the_last_lane_only(emu):
    rng = np.random.default_rng(6)
    n = 128
    bins = [[int(v) for v in rng.integers(0, T, 9)] for _ in range(n)]
    A = poly_array(bins, n)
    for slot in (63, 127):
        pts = [bins[slot][3], (bins[slot][3] + 1) % T, bins[slot][8]]
        got, stats = run_lookup(emu, A, [[p] for p in pts], [slot] * 3)
        assert got == model_flags(A, [[p] for p in pts], [slot] * 3) == [1, int(horner([int(v) for v in A[:, slot]], pts[1]) == 0), 1]
        assert stats == [1, 3, 3]
    # one entry across the tile border, ending in the last slot; other values of R give the same answers
    felts = [[bins[62 + j][j] for j in range(4)], [bins[124 + j][0] for j in range(3)] + [1]]
    start = [62, 124]
    want = model_flags(A, felts, start)
    for r in (1, 4, 8, 16):
        assert run_lookup(emu, A, felts, start, r)[0] == want


def test_lookup_refuses_an_entry_beyond_the_last_slot(emu):
    A = poly_array([[1]] * 64, 64)
    felts = np.array([[1, 1]], dtype=np.uint64)
    start = np.array([63], dtype=np.uint32)
    flags = np.zeros(2, dtype=np.uint8)
    rc = emu.emu_bins_lookup(C.c_uint64(T), vp(A), C.c_uint64(64), C.c_uint32(1), vp(felts), vp(start), C.c_uint64(1), C.c_uint32(2), C.c_int(R),
                             vp(flags), None)
    assert rc == -1 and b"beyond" in emu.emu_last_error()


# ------------------------------------------------------------------------------------------------------------- placement
def model_place(bundles, ins, rem, F, bins, max_items):
    """The reference's loops on bins kept as lists.  bundles: per BinBundle a list of `bins` lists (None: not a bin), in cache order.
    ins / rem: lists of (start, felts).  -> dict of everything emu_place_entries returns."""
    def holds(b, e):
        s, f = e
        return all(b[s + j] is not None and f[j] in b[s + j] for j in range(F))
    given = len(bundles)
    present_ins = [[holds(b, e) for e in ins] for b in bundles]        # as the lookup sees it: before the call
    work = [[None if x is None else list(x) for x in b] for b in bundles]
    rem_lists = [dict() for _ in bundles]
    ins_lists = [dict() for _ in bundles]
    rem_status, rem_target = [], []
    for s, f in rem:
        where = next((i for i, b in enumerate(bundles) if holds(b, (s, f))), None)
        if where is None:
            rem_status.append(NOT_FOUND); rem_target.append(NONE)
            continue
        for j in range(F):
            if f[j] in work[where][s + j]:
                work[where][s + j].remove(f[j])
            rem_lists[where].setdefault(s + j, []).append(f[j])
        rem_status.append(REMOVED); rem_target.append(where)
    state = [REPLACED if rem_lists[i] else UNCHANGED for i in range(given)]
    for i, b in enumerate(work):
        if all(not x for x in b):
            state[i] = EMPTY
    ins_status, ins_target, placed = [], [], {}
    for e, (s, f) in enumerate(ins):
        dup = next((i for i in range(given) if present_ins[i][e]), None)
        if dup is None:
            dup = placed.get((s, tuple(f)))
        if dup is not None:
            ins_status.append(DUPLICATE); ins_target.append(dup)
            continue
        target = None
        for i in reversed(range(len(work))):               # rbegin
            if i < given and state[i] == EMPTY:
                continue
            if any(work[i][s + j] is None for j in range(F)):
                continue
            if max(len(work[i][s + j]) + 1 for j in range(F)) < max_items:
                target = i
                break
        if target is None:
            work.append([[] for _ in range(bins)])
            ins_lists.append(dict())
            target = len(work) - 1
        for j in range(F):
            work[target][s + j].append(f[j])
            ins_lists[target].setdefault(s + j, []).append(f[j])
        if target < given:
            state[target] = REPLACED
        ins_status.append(INSERTED); ins_target.append(target)
        placed[(s, tuple(f))] = target
    return dict(ins_status=ins_status, ins_target=ins_target, rem_status=rem_status, rem_target=rem_target, state=state,
                n_new=len(work) - given, ins_lists=ins_lists, rem_lists=rem_lists + [dict()] * (len(work) - given), final=work)


def run_place(emu, bundles, ins, rem, F, bins, max_items, t=T):
    nb, ni, nr = len(bundles), len(ins), len(rem)
    counts = np.array([[NONE if x is None else len(x) for x in b] for b in bundles], dtype=np.uint32).reshape(nb, bins)

    def pres(entries):
        return np.array([[all(b[s + j] is not None and f[j] in b[s + j] for j in range(F)) if s + F <= bins else 0 for s, f in entries]
                         for b in bundles], dtype=np.uint8).reshape(nb, len(entries))
    fi = np.array([f for _, f in ins], dtype=np.uint64).reshape(ni, F)
    si = np.array([s for s, _ in ins], dtype=np.uint32)
    fr = np.array([f for _, f in rem], dtype=np.uint64).reshape(nr, F)
    sr = np.array([s for s, _ in rem], dtype=np.uint32)
    pi, pr = pres(ins), pres(rem)
    stride = ni + nr + 1
    out32 = [np.zeros(max(k, 1), dtype=np.uint32) for k in (ni, ni, nr, nr, nb)]
    n_new = C.c_uint32()
    ic, rc_ = np.zeros((nb + ni, bins), dtype=np.uint32), np.zeros((nb + ni, bins), dtype=np.uint32)
    ir, rr = np.zeros((nb + ni, bins, stride), dtype=np.uint64), np.zeros((nb + ni, bins, stride), dtype=np.uint64)
    rc = emu.emu_place_entries(C.c_uint32(nb), C.c_uint32(bins), C.c_uint32(F), C.c_uint64(t), C.c_uint32(max_items), vp(counts), vp(pi), vp(pr),
                               vp(fi), vp(si), C.c_uint64(ni), vp(fr), vp(sr), C.c_uint64(nr), *[vp(a) for a in out32], C.byref(n_new),
                               C.c_uint32(stride), vp(ic), vp(ir), vp(rc_), vp(rr))
    if rc != 0:
        return rc, emu.emu_last_error().decode()
    total = nb + n_new.value

    def lists(cnt, roots):
        return [{s: [int(v) for v in roots[b, s, :cnt[b, s]]] for s in range(bins) if cnt[b, s]} for b in range(total)]
    return 0, dict(ins_status=[int(v) for v in out32[0][:ni]], ins_target=[int(v) for v in out32[1][:ni]], rem_status=[int(v) for v in out32[2][:nr]],
                   rem_target=[int(v) for v in out32[3][:nr]], state=[int(v) for v in out32[4][:nb]], n_new=n_new.value,
                   ins_lists=lists(ic, ir), rem_lists=lists(rc_, rr))


def check_place(emu, bundles, ins, rem, F=2, bins=6, max_items=4):
    rc, got = run_place(emu, bundles, ins, rem, F, bins, max_items)
    assert rc == 0, got
    want = model_place(bundles, ins, rem, F, bins, max_items)
    final = want.pop("final")
    assert got == want
    return want, final


def filled(bins, sizes, base=1000):
    """a BinBundle whose bin s holds sizes[s] distinct values (None: not a bin)"""
    return [None if c is None else [base + 100 * s + k for k in range(c)] for s, c in zip(range(bins), sizes)]


def test_place_newest_first(emu):
    b0, b1 = filled(6, [1] * 6), filled(6, [1] * 6, base=5000)
    want, _ = check_place(emu, [b0, b1], [(0, [7, 8])], [])
    assert want["ins_target"] == [1] and want["state"] == [UNCHANGED, REPLACED] and want["n_new"] == 0
    # the newest has no room at that place: the one before it takes the entry
    b1 = filled(6, [3, 1, 1, 1, 1, 1], base=5000)
    want, _ = check_place(emu, [b0, b1], [(0, [7, 8]), (2, [7, 8])], [])
    assert want["ins_target"] == [0, 1] and want["state"] == [REPLACED, REPLACED]
    # a slot that is not a bin cannot take a part
    b1 = filled(6, [1, None, 1, 1, 1, 1], base=5000)
    want, _ = check_place(emu, [b0, b1], [(0, [7, 8]), (1, [7, 8]), (2, [7, 8])], [])
    assert want["ins_target"] == [0, 0, 1]


@pytest.mark.parametrize("size,fits", [(2, True), (3, False), (4, False)])
def test_place_strict_inequality(emu, size, fits):
    """max_items_per_bin = 4: a bin at max - 2 takes one more (2 + 1 < 4), at max - 1 and at max it does not"""
    b0 = filled(6, [0, size, 0, 0, 0, 0])
    want, final = check_place(emu, [b0], [(0, [7, 8])], [], max_items=4)
    assert want["ins_status"] == [INSERTED]
    assert want["ins_target"] == [0 if fits else 1] and want["n_new"] == (0 if fits else 1)
    assert max(len(x) for b in final for x in b) <= max(size, 3)


def test_place_the_first_of_the_batch_takes_the_room(emu):
    b0 = filled(6, [2, 2, 0, 0, 0, 0])
    want, final = check_place(emu, [b0], [(0, [7, 8]), (0, [9, 10]), (1, [11, 12]), (2, [13, 14])], [], max_items=4)
    assert want["ins_target"] == [0, 1, 1, 1] and want["n_new"] == 1
    assert want["ins_lists"][1] == {0: [9], 1: [10, 11], 2: [12, 13], 3: [14]}


def test_place_overflow_into_one_and_into_two_new_bundles(emu):
    full = filled(6, [3] * 6)
    want, _ = check_place(emu, [full], [(0, [1, 2]), (0, [3, 4]), (2, [5, 6]), (4, [7, 8])], [], max_items=4)
    assert want["n_new"] == 1 and want["ins_target"] == [1, 1, 1, 1] and want["state"] == [UNCHANGED]
    # max_items_per_bin = 2 leaves one item per bin: the second entry at a place opens the next BinBundle, the third goes back to ... the newest
    want, _ = check_place(emu, [filled(6, [1] * 6)], [(0, [1, 2]), (0, [3, 4]), (2, [5, 6]), (0, [9, 9])], [], max_items=2)
    assert want["n_new"] == 3 and want["ins_target"] == [1, 2, 2, 3]
    # no BinBundle given at all
    want, _ = check_place(emu, [], [(0, [1, 2]), (1, [3, 4])], [], max_items=3)
    assert want["n_new"] == 1 and want["ins_target"] == [0, 0]
    want, _ = check_place(emu, [], [(0, [1, 2]), (1, [3, 4])], [], max_items=2)
    assert want["n_new"] == 2 and want["ins_target"] == [0, 1]


def test_place_a_removal_makes_room_and_removals_take_the_first_holder(emu):
    b0, b1 = filled(6, [3, 3, 1, 1, 1, 1]), filled(6, [3, 3, 1, 1, 1, 1], base=5000)
    gone = (0, [b1[0][1], b1[1][2]])
    want, final = check_place(emu, [b0, b1], [(0, [7, 8])], [gone], max_items=4)
    assert want["rem_status"] == [REMOVED] and want["rem_target"] == [1]
    assert want["ins_target"] == [1] and want["n_new"] == 0 and want["state"] == [UNCHANGED, REPLACED]
    # without the removal it needs a new BinBundle
    assert check_place(emu, [b0, b1], [(0, [7, 8])], [], max_items=4)[0]["n_new"] == 1
    # an entry that two BinBundles hold leaves the first; one that nobody holds is reported and changes nothing
    both = (2, [b0[2][0], b0[3][0]])
    b1[2].append(both[1][0]); b1[3].append(both[1][1])
    want, _ = check_place(emu, [b0, b1], [], [both, (4, [1, 2]), (4, [b0[4][0], 2])], max_items=4)
    assert want["rem_status"] == [REMOVED, NOT_FOUND, NOT_FOUND] and want["rem_target"] == [0, NONE, NONE]
    assert want["state"] == [REPLACED, UNCHANGED] and want["rem_lists"][1] == {}


def test_place_empty_bundle_is_dropped_and_takes_nothing(emu):
    b0 = filled(6, [1, 1, 0, 0, 0, 0])
    b1 = filled(6, [0, 0, 1, 1, 0, 0], base=5000)
    rem = [(2, [b1[2][0], b1[3][0]])]
    want, _ = check_place(emu, [b0, b1], [(4, [7, 8])], rem, max_items=4)
    assert want["state"] == [REPLACED, EMPTY] and want["ins_target"] == [0]
    want, _ = check_place(emu, [b1], [(4, [7, 8])], rem, max_items=4)
    assert want["state"] == [EMPTY] and want["ins_target"] == [1] and want["n_new"] == 1


def test_place_both_kinds_of_duplicate(emu):
    b0, b1 = filled(6, [1] * 6), filled(6, [1] * 6, base=5000)
    held = (1, [b0[1][0], b0[2][0]])
    false_positive = (3, [b1[3][0], b1[4][0]])             # (with real items the two parts would come from different items)
    fresh = (0, [7, 8])
    want, _ = check_place(emu, [b0, b1], [held, fresh, false_positive, fresh, (0, [7, 9])], [], max_items=4)
    assert want["ins_status"] == [DUPLICATE, INSERTED, DUPLICATE, DUPLICATE, INSERTED]
    assert want["ins_target"] == [0, 1, 1, 1, 1]
    assert want["ins_lists"][1] == {0: [7, 7], 1: [8, 9]}


def test_place_refusals(emu):
    b0 = filled(6, [1] * 6)
    e = (0, [b0[0][0], b0[1][0]])
    for ins, rem, text in (([e], [e], "removal list too"), ([], [e, (1, [5, 5]), e], "twice"), ([(0, [T, 1])], [], "not reduced"),
                           ([], [(0, [1, T + 3])], "not reduced"), ([(5, [1, 2])], [], "exceeds bins_per_bundle"),
                           ([], [(6, [1, 2])], "exceeds bins_per_bundle")):
        rc, msg = run_place(emu, [b0], ins, rem, 2, 6, 4)
        assert rc == -1 and text in msg, (rc, msg)
    # the same entry twice in the INSERT list is no refusal (the second is a duplicate), nor is the same value at another start bin
    rc, got = run_place(emu, [b0], [(0, [1, 2]), (0, [1, 2])], [(1, list(e[1]))], 2, 6, 4)
    assert rc == 0 and got["ins_status"] == [INSERTED, DUPLICATE] and got["rem_status"] == [NOT_FOUND]


def test_place_random_batches_against_the_model(emu):
    rng = np.random.default_rng(77)
    for trial in range(40):
        bins, F, max_items = 8, int(rng.integers(1, 4)), int(rng.integers(2, 6))
        nb = int(rng.integers(0, 4))
        bundles = [[None if rng.random() < 0.1 else [int(v) for v in rng.choice(50, size=int(rng.integers(0, max_items)), replace=False)]
                    for _ in range(bins)] for _ in range(nb)]
        def entry():
            s = int(rng.integers(0, bins - F + 1))
            if nb and rng.random() < 0.5:                  # assembled from what some BinBundle holds
                b = bundles[int(rng.integers(0, nb))]
                if all(b[s + j] for j in range(F)):
                    return (s, [b[s + j][int(rng.integers(0, len(b[s + j])))] for j in range(F)])
            return (s, [int(v) for v in rng.integers(0, 50, F)])
        rem = []
        for _ in range(int(rng.integers(0, 6))):
            e = entry()
            if e not in rem:
                rem.append(e)
        ins = [e for e in (entry() for _ in range(int(rng.integers(0, 10)))) if e not in rem]
        # two removals that share a value a bin holds once are the update's to refuse; the model of this file keeps out of that
        if len(set((s + j, f[j]) for s, f in rem for j in range(F))) != sum(F for _ in rem):
            continue
        check_place(emu, bundles, ins, rem, F=F, bins=bins, max_items=max_items)
