"""The grouping kernels of apsu_amd/csrc/kernels_bucket.hip one at a time: a model of every kernel stated from its definition (not from its
loops), the cases at which each can go wrong, and the checks that both tiers run -- the CPU tier through the per-kernel entry points of
the emulation (test_bucket_step_model_cpu.py), the GPU through the steps behind apsu_he_debug_run_step (test_gpu_bucket_steps.py).

A tier is a RUNNER: an object with one method per kernel that takes numpy uint64 arrays (a 32-bit array travels one value per 64-bit
word, as in the steps) and returns the in/out arrays as the kernel left them:
  count(locs [count][H], tile, tile_cnt) -> tile_cnt          keys(locs, tile, tile_base, keys) -> keys
  scan(vals [n], out [n + 1], sum [1] or None) -> out, sum     hist(keys, total, tile, batch, shift, width, hist, wave_cnt) -> hist, wave_cnt
  scatter(keys, total, tile, batch, shift, width, scanned, wave_cnt, out) -> out
  offsets(keys, total, T, out [T + 2]) -> out                  order(keys, total, out [room]) -> out
  gather(items [count][2], order [room], total, out [room][2]) -> out
Every comparison is exact.  A word the kernel must not write holds POISON before and after."""
import bisect

import numpy as np

WAVE, WAVES, SCAN_STEP = 64, 4, 8192                       # bucket_plan.h: BUCKET_WAVE, BUCKET_WAVES, BUCKET_SCAN_T * BUCKET_SCAN_PER_LANE
POISON = 0xDEADBEEFDEADBEEF
POISON32 = 0xDEADBEEF
M64 = (1 << 64) - 1
U = np.uint64


def u64(x):
    return np.ascontiguousarray(x, dtype=np.uint64)


def poisoned(words, value=POISON):
    return np.full(words, value, dtype=np.uint64)


# ------------------------------------------------------------------------------------------------------------- the models
def first_use(locs):
    """[count][H] bool: entry (i, h) survives iff no g < h has locs[i][g] == locs[i][h]"""
    locs = np.asarray(locs)
    return np.stack([~(locs[:, :h] == locs[:, h:h + 1]).any(axis=1) for h in range(locs.shape[1])], axis=1)


def count_model(locs, tile):
    """tile_cnt[t] = the surviving entries of items t tile .. t tile + tile - 1"""
    per_item = first_use(locs).sum(axis=1)
    return u64([per_item[a:a + tile].sum() for a in range(0, len(locs), tile)])


def keys_model(locs, tile, tile_base, keys):
    """the keys loc << 32 | i of tile t's surviving entries in (i, h) order from tile_base[t] on; every other word of `keys` stays"""
    out, keep = keys.copy(), first_use(locs)
    for t, a in enumerate(range(0, len(locs), tile)):
        i, h = np.nonzero(keep[a:a + tile])                # row-major: (i, h) order
        mine = (u64(locs[a:a + tile][i, h]) << U(32)) | u64(i + a)
        out[int(tile_base[t]):int(tile_base[t]) + len(mine)] = mine
    return out


def scan_model(vals):
    """-> (the exclusive sums, the sum of all) modulo 2^64: numpy's cumsum over Python integers"""
    if not len(vals):
        return u64([]), 0
    inc = np.cumsum(np.asarray([int(v) for v in vals], dtype=object))
    return u64([0] + [int(x) & M64 for x in inc[:-1]]), int(inc[-1]) & M64


def tile_len(total, tile, t):
    return max(0, min(tile, total - t * tile))


def wave_run(tile, length, w):
    """bucket_wave_run: wave w owns keys [begin, end) of its tile, a quarter of the tile cut at the tile's keys"""
    run = tile // WAVES
    return min(w * run, length), min(w * run + run, length)


def digits_of(keys, shift, width):
    return ((keys >> U(shift)) & U((1 << width) - 1)).astype(np.int64)


def hist_model(keys, total, tile, batch, shift, width):
    """hist[d][t] = the keys of tile t below total with digit d; wave_cnt[t][w][d] = those of them in wave w's run"""
    D = 1 << width
    hist, wave_cnt = np.zeros((D, batch), dtype=np.uint64), np.zeros((batch, WAVES, D), dtype=np.uint64)
    for t in range(batch):
        length = tile_len(total, tile, t)
        dg = digits_of(keys[t * tile:t * tile + length], shift, width)
        hist[:, t] = np.bincount(dg, minlength=D)
        for w in range(WAVES):
            b, e = wave_run(tile, length, w)
            wave_cnt[t, w] = np.bincount(dg[b:e], minlength=D)
    return hist.reshape(-1), wave_cnt.reshape(-1)


def scatter_places(keys, total, tile, batch, shift, width, scanned, wave_cnt):
    """-> (place of every key below total, those keys): scanned[d][t] + the given wave_cnt[t][ww][d] of the waves ww < w + the key's rank
    among the equal digits earlier in its wave's run -- from the GIVEN arrays, whatever they hold"""
    D = 1 << width
    scanned, wave_cnt = scanned.reshape(D, batch).astype(np.int64), wave_cnt.reshape(batch, WAVES, D).astype(np.int64)
    places, moved = [], []
    for t in range(batch):
        length = tile_len(total, tile, t)
        for w in range(WAVES):
            b, e = wave_run(tile, length, w)
            mine = keys[t * tile + b:t * tile + e]
            dg = digits_of(mine, shift, width)
            rank = np.zeros(len(dg), dtype=np.int64)
            if len(dg):                                        # the position of each key among the run's keys of its digit (a stable sort by digit)
                by_digit = np.argsort(dg, kind="stable")
                starts = np.concatenate([[0], np.nonzero(np.diff(dg[by_digit]))[0] + 1])
                rank[by_digit] = np.arange(len(dg)) - np.repeat(starts, np.diff(np.concatenate([starts, [len(dg)]])))
            places.append(scanned[dg, t] + wave_cnt[t, :w, :].sum(axis=0)[dg] + rank)
            moved.append(mine)
    return (np.concatenate(places), np.concatenate(moved)) if places else (np.zeros(0, dtype=np.int64), u64([]))


def scatter_model(keys, total, tile, batch, shift, width, scanned, wave_cnt, out):
    places, moved = scatter_places(keys, total, tile, batch, shift, width, scanned, wave_cnt)
    want = out.copy()
    assert len(set(places.tolist())) == len(places) and (len(places) == 0 or places.max() < len(out))     # (the case is well formed)
    want[places] = moved
    return want


def offsets_model(keys, total, T):
    """offsets[l] = the keys among the first `total` below l << 32, l <= T"""
    ks = [int(k) for k in keys[:total]]
    return u64([bisect.bisect_left(ks, l << 32) for l in range(T + 1)])


def order_model(keys, total):
    return keys[:total] & U(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------------------- the scan
SCAN_LENGTHS = [0, 1, 7, 8, 9, 511, 512, 513, 8191, 8192, 8193, 16384, 3 * 8192 + 5, 100003]


def scan_values(n):
    return [("zeros", np.zeros(n, dtype=np.uint64)), ("ones", np.ones(n, dtype=np.uint64)), ("all 0xFFFFFFFF", np.full(n, 0xFFFFFFFF, dtype=np.uint64)),
            ("random", np.random.default_rng(n).integers(0, 1 << 32, n, dtype=np.uint64))]


def check_scan(run, lengths=SCAN_LENGTHS):
    """every length x every value pattern, with and without the sum pointer; the guard behind out[n - 1] and (without the pointer) the sum
    word keep their poison; n = 0 writes the sum alone.  -> the number of launches checked"""
    done = 0
    # all 0xFFFFFFFF: a lane's eight words pass 2^32, so does the carry after one step, and the longest total passes 2^48
    assert 0xFFFFFFFF * 8 > 1 << 32 and 0xFFFFFFFF * SCAN_STEP > 1 << 32 and 0xFFFFFFFF * max(SCAN_LENGTHS) > 1 << 48
    for n in lengths:
        for name, vals in scan_values(n):
            want, want_sum = scan_model(vals)
            for with_sum in (True, False):
                out, s = run.scan(vals, poisoned(n + 1), poisoned(1) if with_sum else None)
                assert (out[:n] == want).all(), ("scan", n, name, with_sum, int(np.nonzero(out[:n] != want)[0][0]))
                assert out[n] == POISON, ("scan: the guard", n, name)
                if with_sum:
                    assert int(s[0]) == want_sum, ("scan: the sum", n, name)
                done += 1
    return done


# ------------------------------------------------------------------------------------------------------------- histogram and scatter
def make_keys(kind, words, shift, width, rng):
    """`words` keys of one kind: how the digit field and the bits around it are filled"""
    D, field = 1 << width, ((1 << width) - 1) << shift
    rand = rng.integers(0, 1 << 63, words, dtype=np.uint64) * U(2) + rng.integers(0, 2, words, dtype=np.uint64)
    dg = rng.integers(0, D, words, dtype=np.uint64)
    if kind == "random":
        return rand
    if kind == "others set":                                # ~digit_field | digit
        return U(M64 ^ field) | (dg << U(shift))
    if kind == "others clear":
        return dg << U(shift)
    if kind == "one digit":                                 # 64 peers in every round
        return (rand & U(M64 ^ field)) | U((D // 2) << shift)
    if kind == "digits 0 and D - 1":
        return (rand & U(M64 ^ field)) | (np.where(rng.integers(0, 2, words) == 1, D - 1, 0).astype(np.uint64) << U(shift))
    if kind == "digit = lane":
        return (rand & U(M64 ^ field)) | ((np.arange(words, dtype=np.uint64) % U(WAVE) % U(D)) << U(shift))
    raise ValueError(kind)


KEY_KINDS = ["random", "others set", "others clear", "one digit", "digits 0 and D - 1", "digit = lane"]


def totals_of(tile, batch):
    q = tile // 4
    ts = {0, 1, 63, 64, 65, q - 1, q, q + 1, q + 65, tile - 1, tile, tile + 1, batch * tile}
    if batch >= 3:
        ts.add((batch - 2) * tile)                          # the last two tiles of the grid are empty
        ts.add((batch - 2) * tile - 5)
    return sorted(x for x in ts if x <= batch * tile)


def hist_cases():
    """(name, keys, total, tile, batch, shift, width)"""
    out = []
    for tile, batch in ((256, 1), (256, 3), (256, 40), (512, 1), (512, 3), (8192, 1), (8192, 3)):      # a wave's run: 1, 2 and 32 rounds
        rng = np.random.default_rng(tile + batch)
        keys = make_keys("random", tile * batch, 32, 8, rng)
        for total in totals_of(tile, batch):
            out.append(("tile %d x %d, total %d" % (tile, batch, total), keys, total, tile, batch, 32, 8))
    tile, batch = 256, 3
    total = 2 * tile + 70
    rng = np.random.default_rng(5)
    for shift, widths in ((32, range(1, 9)), (40, range(1, 9)), (56, range(1, 9)), (63, (1,))):
        for width in widths:
            out.append(("shift %d width %d" % (shift, width), make_keys("random", tile * batch, shift, width, rng), total, tile, batch, shift, width))
    for tile in (256, 512):
        for shift, width in ((40, 8), (33, 3)):
            for kind in KEY_KINDS:
                rng = np.random.default_rng(tile + width)
                out.append(("%s, tile %d, shift %d width %d" % (kind, tile, shift, width), make_keys(kind, tile * 3, shift, width, rng),
                            2 * tile + tile // 4 + 7, tile, 3, shift, width))
    return out


def check_hist(run, cases=None):
    done = 0
    for name, keys, total, tile, batch, shift, width in cases or hist_cases():
        D = 1 << width
        want_h, want_w = hist_model(keys, total, tile, batch, shift, width)
        hist, wave_cnt = run.hist(keys, total, tile, batch, shift, width, poisoned(D * batch, POISON32), poisoned(batch * WAVES * D, POISON32))
        assert (hist == want_h).all(), ("hist", name)
        assert (wave_cnt == want_w).all(), ("wave_cnt", name)
        assert int(want_h.sum()) == total
        for t in range(batch):                              # a tile beyond the total: zeros, written
            if tile_len(total, tile, t) == 0:
                assert (hist.reshape(D, batch)[:, t] == 0).all() and (wave_cnt.reshape(batch, -1)[t] == 0).all(), ("hist: an empty tile", name)
        done += 1
    return done


def true_scanned(hist):
    return scan_model(hist)[0]


def check_scatter(run, cases=None):
    """per case three launches: (a) the true scan of the true histogram: a permutation of the keys below total, nothing behind;
    (b) a scanned array with 3 free words in front of every (digit, tile) cell, over poison: every key exactly on its place, every
    other word poison; (c) wave 0's counts one too large: the waves' shares lie one word apart"""
    done = 0
    for name, keys, total, tile, batch, shift, width in cases or hist_cases():
        D = 1 << width
        hist, wave_cnt = hist_model(keys, total, tile, batch, shift, width)
        geom = (keys, total, tile, batch, shift, width)
        # (a)
        scanned = true_scanned(hist)
        room = batch * tile + 1
        want = scatter_model(*geom, scanned, wave_cnt, poisoned(room))
        out = run.scatter(*geom, scanned, wave_cnt, poisoned(room))
        assert (out == want).all(), ("scatter", name)
        assert (want[total:] == POISON).all() and sorted(want[:total].tolist()) == sorted(keys[:total].tolist())
        # (b)
        gaps = scanned + U(3) * (np.arange(D * batch, dtype=np.uint64) + U(1))
        room = batch * tile + 3 * D * batch + 1
        want = scatter_model(*geom, gaps, wave_cnt, poisoned(room))
        out = run.scatter(*geom, gaps, wave_cnt, poisoned(room))
        assert (out == want).all(), ("scatter over gaps", name)
        assert int((want != POISON).sum()) == total or (keys[:total] == U(POISON)).any()
        # (c)
        fat = wave_cnt.reshape(batch, WAVES, D).copy()
        fat[:, 0, :] += U(1)
        wide = scan_model(hist + U(1))[0]                   # every cell one word longer: room for wave 0's extra word
        room = batch * tile + D * batch + 1
        want = scatter_model(*geom, wide, fat.reshape(-1), poisoned(room))
        out = run.scatter(*geom, wide, fat.reshape(-1), poisoned(room))
        assert (out == want).all(), ("scatter with wave 0's counts inflated", name)
        done += 3
    return done


# ------------------------------------------------------------------------------------------------------------- count and keys
def collide(locs, H):
    """items by turns: distinct, h0 = h1, h0 = h2, h1 = h2, all equal (tests/bucket_cases.py)"""
    if H < 3:
        return locs
    kind = np.arange(len(locs)) % 5
    locs[:, 1] = locs[:, 0] + 1
    locs[:, 2] = locs[:, 0] + 2
    locs[kind == 1, 1] = locs[kind == 1, 0]
    locs[kind == 2, 2] = locs[kind == 2, 0]
    locs[kind == 3, 2] = locs[kind == 3, 1]
    locs[kind == 4, 1] = locs[kind == 4, 0]
    locs[kind == 4, 2] = locs[kind == 4, 0]
    return locs


def key_cases():
    """(name, locs [count][H], tile)"""
    out = []
    for tile in (256, 512):
        for H in (1, 3, 8):
            for count in sorted({1, 255, 256, 257, tile - 1, tile, tile + 1, 2 * tile + 3}):
                rng = np.random.default_rng(count * H + tile)
                locs = collide(rng.integers(0, 6552, (count, H)).astype(np.uint64), H)
                if H == 8:
                    locs[::3, 7] = locs[::3, 4]             # a collision among the later functions too
                out.append(("%d items, H = %d, tile %d" % (count, H, tile), locs, tile))
    return out


def check_count_and_keys(run, cases=None):
    done = 0
    for name, locs, tile in cases or key_cases():
        count, H = locs.shape
        tiles = -(-count // tile)
        want_cnt = count_model(locs, tile)
        cnt = run.count(locs, tile, poisoned(tiles, POISON32))
        assert (cnt == want_cnt).all(), ("count", name)
        assert H > 1 or int(want_cnt.sum()) == count
        # the caller's bases: 5 free words in front of every tile's range
        base = scan_model(want_cnt)[0] + U(5) * (np.arange(tiles, dtype=np.uint64) + U(1))
        room = int(want_cnt.sum()) + 5 * tiles + 5
        want = keys_model(locs, tile, base, poisoned(room))
        keys = run.keys(locs, tile, base, poisoned(room))
        assert (keys == want).all(), ("keys", name)
        assert int((want != POISON).sum()) == int(want_cnt.sum())
        done += 1
    return done


# ------------------------------------------------------------------------------------------------------------- offsets, order, gather
TABLE_SIZES = [1, 2, 255, 256, 257, 65537]


def sorted_key_cases():
    """(name, keys, total, T): ascending keys below `total`, garbage behind"""
    out = []
    for T in TABLE_SIZES:
        rng = np.random.default_rng(T)
        for total, given in ((0, 0), (0, 9), (1, 1), (257, 257), (257, 300), (100, 257)):
            spreads = [("random", rng.integers(0, T, given)), ("every key in the last bucket", np.full(given, T - 1))]
            if T >= 255:
                spreads.append(("empty buckets at both ends", rng.integers(T // 3, T // 3 + 5, given)))
            for name, loc in spreads:
                keys = (u64(loc) << U(32)) | rng.integers(0, 1 << 32, given, dtype=np.uint64)
                keys[:total] = np.sort(keys[:total])
                keys[total:] = rng.integers(0, 1 << 32, given - total, dtype=np.uint64)      # garbage: bucket 0, unsorted
                out.append(("%s, T = %d, %d of %d keys" % (name, T, total, given), keys, total, T))
    return out


def check_offsets_and_order(run, cases=None):
    done = 0
    for name, keys, total, T in cases or sorted_key_cases():
        out = run.offsets(keys, total, T, poisoned(T + 2))
        assert (out[:T + 1] == offsets_model(keys, total, T)).all(), ("offsets", name)
        assert out[T + 1] == POISON and out[T] == total, ("offsets: the guard", name)
        room = len(keys) + 1
        order = run.order(keys, total, poisoned(room, POISON32))
        assert (order[:total] == order_model(keys, total)).all() and (order[total:] == POISON32).all(), ("order", name)
        done += 1
    return done


def gather_cases():
    """(name, items [count][2], order [room], total)"""
    out = []
    walking = u64([[(1 << b) & M64, (1 << b) >> 64] for b in range(128)])
    rng = np.random.default_rng(16)
    for name, items in (("all 0xFF", np.full((300, 2), M64, dtype=np.uint64)), ("a walking one", walking),
                        ("random", rng.integers(0, 1 << 63, (257, 2), dtype=np.uint64) * U(2) + U(1)), ("one item", u64([[3, 4]]))):
        count = len(items)
        for room, total in ((1, 0), (1, 1), (257, 257), (300, 257), (300, 0), (1025, 1000)):
            order = rng.integers(0, count, room, dtype=np.uint64)              # with repeats
            order[total:] = POISON32                                            # beyond total: never read
            if total >= 2:
                order[1] = order[0]
            out.append(("%s, %d of %d" % (name, total, room), items, order, total))
    return out


def check_gather(run, cases=None):
    done = 0
    for name, items, order, total in cases or gather_cases():
        room = len(order)
        out = run.gather(items, order, total, poisoned(2 * room).reshape(room, 2))
        assert (out[:total] == items[order[:total].astype(np.int64)]).all(), ("gather", name)
        assert (out[total:] == POISON).all(), ("gather: beyond total", name)
        done += 1
    return done


# ------------------------------------------------------------------------------------------------------------- the pipeline, model by model
def pipeline_model(locs, T, tile, widths):
    """launch_bucket_sort restated with the models above: locs uint32 [count][H], widths = the digit plan's -> (offsets, order)"""
    locs = u64(locs)
    count, H = locs.shape
    cnt = count_model(locs, tile)
    base, total = scan_model(cnt)
    keys = keys_model(locs, tile, base, poisoned(count * H))
    batch, shift = -(-(count * H) // tile), 32
    for width in widths:
        hist, wave_cnt = hist_model(keys, total, tile, batch, shift, width)
        keys = scatter_model(keys, total, tile, batch, shift, width, true_scanned(hist), wave_cnt, poisoned(count * H))
        shift += width
    return offsets_model(keys, total, T), order_model(keys, total).astype(np.uint32)
