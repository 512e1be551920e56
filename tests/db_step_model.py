"""The resident-database kernels (apsu_amd/csrc/kernels_db.hip, kernels_roots.hip) stated on Python integers,
each from its definition and not from the kernel's loop structure: product of linear factors and polynomial product through ONE
big-integer multiplication (Kronecker substitution), synthetic division with its remainder, Horner, the per-slot convolution, a count
as the index of the top non-zero coefficient, ragged rows, the multiset of roots with multiplicities (a search over the whole field).

Arrays are poly[rows][n]: column s is the polynomial of bin (slot) s, coefficient d in row d.  Functions take and return numpy uint64
arrays or lists of Python ints; t is the plain modulus.  tests/test_db_step_model_cpu.py holds this file to the oracle and to the CPU
emulation of the kernels; tests/test_gpu_db_kernel_steps.py holds the kernels to it."""
import numpy as np

NONE = 0xFFFFFFFF                                         # LOOKUP_NONE: the count of a slot that is not a bin; no point in a plan's cell
NO_WORD = (1 << 64) - 1                                   # a status word nobody lowered
LANES = 64
MERGE_K = 8
EVAL_ROWS = 8
LOOKUP_R = 8
FOLD_CAP = 1024
SLOTS = (1, 2, 4, 8, 16, 24, 32, 48, 64, 96, 128)          # the instances of k_polyn_with_roots / k_bins_update


def ints(a):
    return [int(v) for v in a]


def U(rows):
    return np.array(rows, dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------- polynomials
def poly_mul(a, b, t):
    """a b mod t for coefficient lists (ascending): both packed into one integer each, one product, no sum carries over"""
    if not a or not b:
        return []
    width = (2 * t.bit_length() + min(len(a), len(b)).bit_length() + 7) // 8 + 1
    pa = int.from_bytes(b"".join(int(v).to_bytes(width, "little") for v in a), "little")
    pb = int.from_bytes(b"".join(int(v).to_bytes(width, "little") for v in b), "little")
    prod = (pa * pb).to_bytes(width * (len(a) + len(b)), "little")
    return [int.from_bytes(prod[i * width:(i + 1) * width], "little") % t for i in range(len(a) + len(b) - 1)]


def poly_from_roots(roots, t, lead=1):
    """lead prod (x - r), ascending coefficients: a balanced tree of products"""
    level = [[(-int(r)) % t, 1] for r in roots]
    if not level:
        return [lead % t]
    while len(level) > 1:
        level = [poly_mul(level[i], level[i + 1], t) if i + 1 < len(level) else level[i] for i in range(0, len(level), 2)]
    return [c * lead % t for c in level[0]]


def divide(p, r, t):
    """p / (x - r) -> (quotient, remainder): q_{k-1} = p_k + r q_k from the top down"""
    q, acc = [0] * (len(p) - 1), 0
    for k in range(len(p) - 1, 0, -1):
        acc = (p[k] + r * acc) % t
        q[k - 1] = acc
    return q, (p[0] + r * acc) % t


def horner(p, x, t):
    acc = 0
    for c in reversed(p):
        acc = (acc * x + c) % t
    return acc


def top_of(col):
    """index of the highest non-zero coefficient, -1 for the zero polynomial"""
    for d in range(len(col) - 1, -1, -1):
        if col[d]:
            return d
    return -1


def count_of(col):
    top = top_of(col)
    return NONE if top < 0 else top


# ---------------------------------------------------------------------------------------------------------------- the steps
def slots_instance(slots):
    """the register-slot instance a launcher takes for `slots` slots of 64 coefficients; None: the serial fallback"""
    for s in SLOTS:
        if slots <= s:
            return s
    return None


def polyn_with_roots(roots, counts, stride, max_deg, n, t):
    """roots [bins][stride], counts [bins] -> poly [max_deg + 1][n]: bin s holds prod_{r < counts[s]} (x - roots[s][r]), 0 above"""
    out = np.zeros((max_deg + 1, n), dtype=np.uint64)
    for s, c in enumerate(ints(counts)):
        p = poly_from_roots(ints(roots[s * stride:s * stride + c]), t)
        out[:len(p), s] = U(p)
    return out


def bins_update(poly, touched, ins, ins_counts, ins_stride, rem, rem_counts, rem_stride, t):
    """P_s <- P_s / prod (x - rem) * prod (x - ins) on the touched columns of poly [rows][n].
    -> (poly after, counts_out per touched entry (None where the wave stops), status[0], status[1], the bins that failed).
    A column whose removal fails or that holds the zero polynomial is returned as it came (what the wave-per-bin instances leave; the
    serial fallback leaves such a column unspecified: device.h)."""
    out = poly.copy()
    rows = poly.shape[0]
    counts_out, st0, st1, failed = [], NO_WORD, NO_WORD, []
    for s in ints(touched):
        col = ints(poly[:, s])
        top = top_of(col)
        if top < 0:
            st1 = min(st1, s)
            counts_out.append(None)
            failed.append(s)
            continue
        p = col[:top + 1]
        bad = None
        for r in range(int(rem_counts[s]) if rem_counts is not None else 0):
            p, remainder = divide(p, int(rem[s * rem_stride + r]), t)
            if remainder:
                bad = r
                break
        if bad is not None:
            st0 = min(st0, s << 32 | bad)
            counts_out.append(None)
            failed.append(s)
            continue
        n_ins = int(ins_counts[s]) if ins_counts is not None else 0
        if n_ins:
            p = poly_mul(p, poly_from_roots(ints(ins[s * ins_stride:s * ins_stride + n_ins]), t), t)
        assert len(p) <= rows
        out[:, s] = U(p + [0] * (rows - len(p)))
        counts_out.append(len(p) - 1)
    return out, counts_out, st0, st1, failed


def bin_counts(poly):
    return [count_of(ints(poly[:, s])) for s in range(poly.shape[1])]


def poly_degree(poly):
    return max([0] + [top_of(ints(poly[:, s])) for s in range(poly.shape[1])])


def unlift(x, t, q0):
    """the stored residue mod q_0 of a plaintext coefficient back to its value mod t: v < t stands for itself, v + (q_0 - t) for v"""
    return [v if v < t else v - (q0 - t) for v in ints(x)]


def lookup_plan(felts, start, F, n, R=LOOKUP_R):
    """the layout of bin_lookup.h: per tile of 64 slots rows of 64 cells, row r holding the r-th point of each slot; work items of at
    most R rows -> (work [(tile, row0, nrows)], pts [rows][64], idx [rows][64])"""
    tiles = (n + LANES - 1) // LANES
    per_slot = [[] for _ in range(tiles * LANES)]
    for e, s in enumerate(ints(start)):
        for j in range(F):
            per_slot[s + j].append((int(felts[e * F + j]), e * F + j))
    work, pts, idx = [], [], []
    for tl in range(tiles):
        cells = per_slot[tl * LANES:(tl + 1) * LANES]
        rows, row0 = max(len(c) for c in cells), len(pts)
        for r in range(rows):
            pts.append([c[r][0] if r < len(c) else 0 for c in cells])
            idx.append([c[r][1] if r < len(c) else NONE for c in cells])
        for r in range(0, rows, R):
            work.append((tl, row0 + r, min(R, rows - r)))
    return work, pts, idx


def bins_lookup(poly, work, pts, idx, flags, t):
    """flags[part] = 1 iff the part's point is a root of its slot's polynomial and the slot is a bin (its column is not zero); a part
    no work item names keeps what `flags` held"""
    out = list(flags)
    cols, value = {}, {}
    for tile, row0, nrows in work:
        for r in range(row0, row0 + nrows):
            for lane in range(LANES):
                part = idx[r][lane]
                if part == NONE:
                    continue
                s = tile * LANES + lane
                if s not in cols:
                    cols[s] = ints(poly[:, s])
                key = (s, int(pts[r][lane]))
                if key not in value:
                    value[key] = horner(cols[s], key[1], t)
                out[part] = 1 if any(cols[s]) and value[key] == 0 else 0
    return out


def merge_fold_interval(bits):
    w = (64 if bits <= 32 else 128) - 2 * bits
    return FOLD_CAP if w >= 10 else 1 << w


def bins_merge(A, topsA, B, topsB, rows, t):
    """C [rows][n]: per slot the product of the two columns, each read up to its tile's top (rows above it are not part of the
    operand); a tile with a top of -1 on either side gives 0"""
    n = A.shape[1]
    out = np.zeros((rows, n), dtype=np.uint64)
    for s in range(n):
        ta, tb = int(topsA[s // LANES]), int(topsB[s // LANES])
        if ta < 0 or tb < 0:
            continue
        p = poly_mul(ints(A[:ta + 1, s]), ints(B[:tb + 1, s]), t)[:rows]
        out[:len(p), s] = U(p)
    return out


def merge_largest_sum(a, b, t, K=MERGE_K):
    """the largest unreduced value an accumulator of one slot's merge holds when its sums are reduced once per fold interval: output
    row k gathers a_i b_{k-i} over the steps i of its block's walk (from a multiple of K below max(k0 - top_b, 0) to min(k0 + K - 1,
    top_a), every step counted whether or not it adds anything), reduced before a step when `fold` steps have gone by"""
    fold = merge_fold_interval(t.bit_length())
    ta, tb, worst = len(a) - 1, len(b) - 1, 0
    for k0 in range(0, ta + tb + 1, K):
        i0, i1 = max(k0 - tb, 0) // K * K, min(k0 + K - 1, ta)
        for k in range(k0, min(k0 + K, ta + tb + 1)):
            acc = pending = 0
            for i in range(i0, i1 + 1):
                if pending == fold:
                    acc, pending = acc % t, 0
                pending += 1
                if 0 <= k - i <= tb:
                    acc += a[i] * b[k - i]
                worst = max(worst, acc)
    return worst


def bins_rows(poly, counts, bins):
    """-> (off [bins + 1], the words out[0 .. off[bins])): bin s's coefficients 0 .. counts[s], one bin behind the other"""
    off, out = [0], []
    for s in range(bins):
        c = int(counts[s])
        out += ints(poly[:c + 1, s])
        off.append(len(out))
    return off, out


def bins_eval(poly, counts, x, mask, t):
    """-> (out [n], is_bin [n]): out[s] = sum_{d <= top} poly[d][s] x[s]^d + mask[s], top the largest count of the slot's tile of 64
    (never above the last row; nothing is read for a tile without a bin); is_bin[s] = the slot's count is not NONE"""
    rows, n = poly.shape
    out, is_bin = [], []
    for s in range(n):
        tile = [int(c) for c in counts[s // LANES * LANES:(s // LANES + 1) * LANES]]
        top = min(max([-1] + [c for c in tile if c != NONE]), rows - 1)
        out.append((horner(ints(poly[:top + 1, s]), int(x[s]), t) + (int(mask[s]) if mask is not None else 0)) % t)
        is_bin.append(0 if int(counts[s]) == NONE else 1)
    return out, is_bin


def eval_compare(got, want):
    """got, want [count][n] -> (mismatches, the lowest position << 32 | slot of one, NO_WORD for none)"""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return len(bad), min([int(p) << 32 | int(s) for p, s in bad] + [NO_WORD])


def field_roots(col, t):
    """{root: multiplicity} of the polynomial col (ascending, not zero) over F_t, by trying every element of the field (t < 2^31) and
    dividing the found ones out"""
    assert t < 1 << 31
    top = top_of(col)
    x = np.arange(t, dtype=np.uint64)
    acc = np.zeros(t, dtype=np.uint64)
    tt = np.uint64(t)
    for d in range(top, -1, -1):
        acc = (acc * x + np.uint64(col[d])) % tt
    found = {}
    p = list(col[:top + 1])
    for r in ints(np.nonzero(acc == 0)[0]):
        while len(p) > 1:
            q, remainder = divide(p, r, t)
            if remainder:
                break
            p, found[r] = q, found.get(r, 0) + 1
    return found


def roots_step(poly, t):
    """the occupied bins (count >= 1) in slot order -> [(slot, count, {root: multiplicity})]"""
    out = []
    for s in range(poly.shape[1]):
        col = ints(poly[:, s])
        top = top_of(col)
        if top >= 1:
            out.append((s, top, field_roots(col, t)))
    return out
