"""CPU tier of writing a database in the reference's saved format (apsu_amd/csrc/wire.h: build_bin_bundle, build_receiver_db_header;
apsu_amd/csrc/bin_rows.h: k_bins_rows as emu_bins_rows steps it).  Three checkers hold the writer: the library's own reader, the
independent FlatBuffers model of tests/test_wire_framing.py (extended here with the matching polynomials and the empty label
vectors), and a structural verifier that walks a buffer the way flatbuffers::Verifier does.  All comparisons are exact."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import common
from apsu_amd import wire
import emu_lib
from emu_lib import vp
from test_wire_framing import FbBuilder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "apsu_amd", "csrc")
NONE = 0xFFFFFFFF
MOD = 65537

BINS = [[5, 7, 11], [], [2**40 + 3], list(range(1, 9)), []]


def matching(bins, t=MOD):
    """prod (x - r) mod t per bin, ascending and monic; [1] for an empty bin"""
    out = []
    for b in bins:
        p = [1]
        for r in b:
            q = [0] * (len(p) + 1)
            for i, c in enumerate(p):
                q[i + 1] = (q[i + 1] + c) % t
                q[i] = (q[i] - c * r) % t
            p = q
        out.append(p)
    return out


POLYNS = matching(BINS)
BLOBS = [bytes([d + 1]) * (10 + 7 * d) for d in range(9)]


# --------------------------------------------------------------------------------------------- the model, extended
def model_felt_matrix(B, rows):
    return B.table([("off", B.offset_vector([B.table([("off", B.u64_vector(r))]) for r in rows]))])


def model_bin_bundle(bundle_idx, mod, bins, polyns, blobs, stripped=False, cache=True):
    """BinBundle::save (bin_bundle.cpp:1107-1169) with everything it writes on the unlabeled path"""
    B = FbBuilder()
    cache_t = None
    if cache:
        bi = B.offset_vector([])
        fi = B.offset_vector([])
        bp = B.table([("off", B.offset_vector([B.table([("off", B.byte_vector(b))]) for b in blobs]))])
        fm = model_felt_matrix(B, [] if stripped else polyns)
        cache_t = B.table([("off", fm), ("off", bp), ("off", fi), ("off", bi)])
    labels = B.offset_vector([])
    items = model_felt_matrix(B, [] if stripped else bins)
    root = B.table([("u32", bundle_idx) if bundle_idx else None, ("u64", mod), ("off", items), ("off", labels),
                    ("off", cache_t) if cache_t is not None else None, ("u8", 1) if stripped else None])
    return B.finish_size_prefixed(root)


def model_header(params, key, hashed, item_count, count, compressed, stripped, nonce=0):
    B = FbBuilder()
    hv = B.struct_vector([struct.pack("<QQ", a, b) for a, b in hashed], 8)
    kv = B.byte_vector(key)
    pv = B.byte_vector(params)
    info = struct.pack("<IIQ??", 0, nonce, item_count, compressed, stripped) + bytes(6)
    return B.finish_size_prefixed(B.table([("off", pv), ("struct", info, 8), ("off", kv), ("off", hv), ("u32", count) if count else None]))


# --------------------------------------------------------------------------------------------- the structural verifier
# a schema: list over field ids of (name, kind, required, sub); kinds: u8 u32 u64, struct (sub = (size, align)), bytes, vec_u64,
# vec_struct (sub = (size, align)), table (sub = schema), vec_table (sub = schema)
FELT_ARRAY = [("felts", "vec_u64", True, None)]
FELT_MATRIX = [("rows", "vec_table", True, FELT_ARRAY)]
PLAINTEXT = [("data", "bytes", True, None)]
BATCHED = [("coeffs", "vec_table", True, PLAINTEXT)]
CACHE = [("felt_matching_polyns", "table", True, FELT_MATRIX), ("batched_matching_polyn", "table", True, BATCHED),
         ("felt_interp_polyns", "vec_table", False, FELT_MATRIX), ("batched_interp_polyns", "vec_table", False, BATCHED)]
BIN_BUNDLE = [("bundle_idx", "u32", False, None), ("mod", "u64", False, None), ("item_bins", "table", True, FELT_MATRIX),
              ("label_bins", "vec_table", False, FELT_MATRIX), ("cache", "table", False, CACHE), ("stripped", "u8", False, None)]
RECEIVER_DB = [("params", "bytes", True, None), ("info", "struct", False, (24, 8)), ("oprf_key", "bytes", True, None),
               ("hashed_items", "vec_struct", True, (16, 8)), ("bin_bundle_count", "u32", False, None)]


class Malformed(Exception):
    pass


def verify(buf, schema):
    """walks a size-prefixed buffer as flatbuffers::Verifier would; returns the set of field names seen present"""
    n = len(buf)
    seen = set()

    def need(ok, what):
        if not ok:
            raise Malformed(what)

    def u16(p):
        need(p % 2 == 0 and 0 <= p and p + 2 <= n, "u16 at %d" % p)
        return struct.unpack_from("<H", buf, p)[0]

    def u32(p):
        need(p % 4 == 0 and 0 <= p and p + 4 <= n, "u32 at %d" % p)
        return struct.unpack_from("<I", buf, p)[0]

    def follow(p):
        o = u32(p)
        need(o != 0 and p + o < n, "offset at %d leaves the buffer" % p)
        return p + o

    def vector(p, elem, align):
        cnt = u32(p)
        need(p + 4 + cnt * elem <= n, "vector at %d leaves the buffer" % p)
        need(cnt == 0 or (p + 4) % align == 0, "vector elements at %d are not aligned to %d" % (p + 4, align))
        return cnt

    def table(pos, sch):
        so = struct.unpack("<i", struct.pack("<I", u32(pos)))[0]
        vt = pos - so
        need(0 <= vt and vt + 4 <= n, "vtable of %d out of bounds" % pos)
        vsz, tsz = u16(vt), u16(vt + 2)
        need(vsz >= 4 and vsz % 2 == 0 and vt + vsz <= n, "vtable size")
        need(tsz >= 4 and pos + tsz <= n, "table size")
        for fid, (name, kind, required, sub) in enumerate(sch):
            off = u16(vt + 4 + 2 * fid) if 4 + 2 * fid + 2 <= vsz else 0
            if not off:
                need(not required, "required field %s is absent" % name)
                continue
            seen.add(name)
            p = pos + off
            size, align = {"u8": (1, 1), "u32": (4, 4), "u64": (8, 8)}.get(kind, sub if kind == "struct" else (4, 4))
            need(off + size <= tsz, "field %s leaves its table" % name)
            need(p % align == 0, "field %s at %d is not aligned to %d" % (name, p, align))
            if kind in ("u8", "u32", "u64", "struct"):
                continue
            t = follow(p)
            if kind == "bytes":
                vector(t, 1, 1)
            elif kind == "vec_u64":
                vector(t, 8, 8)
            elif kind == "vec_struct":
                vector(t, sub[0], sub[1])
            elif kind == "table":
                table(t, sub)
            else:
                for i in range(vector(t, 4, 4)):
                    table(follow(t + 4 + 4 * i), sub)

    need(n >= 8 and struct.unpack_from("<I", buf, 0)[0] == n - 4, "size prefix")
    table(follow(4), schema)
    return seen


def test_the_verifier_has_teeth_on_the_writers_output():
    good = wire.build_bin_bundle(3, MOD, BINS, POLYNS, BLOBS)
    assert {"item_bins", "rows", "felts", "felt_matching_polyns", "batched_matching_polyn", "coeffs", "data"} <= verify(good, BIN_BUNDLE)
    with pytest.raises(Malformed):
        verify(good[:-4], BIN_BUNDLE)                                  # size prefix
    with pytest.raises(Malformed):
        verify(good[:4] + b"\xf0\xff\xff\x7f" + good[8:], BIN_BUNDLE)  # root offset out of the buffer
    # a [uint64] whose elements are only 4-aligned: everything behind the root offset moves by one word (offsets are relative)
    B = FbBuilder()
    ok = B.finish_size_prefixed(B.table([("off", B.u64_vector([1, 2, 3]))]))
    assert verify(ok, FELT_ARRAY) == {"felts"}
    bad = bytearray(ok)
    bad[8:8] = b"\0\0\0\0"
    struct.pack_into("<I", bad, 0, len(bad) - 4)
    struct.pack_into("<I", bad, 4, struct.unpack_from("<I", bad, 4)[0] + 4)
    with pytest.raises(Malformed, match="aligned to 8"):
        verify(bytes(bad), FELT_ARRAY)
    with pytest.raises(Malformed, match="required"):
        verify(_empty_table(), FELT_ARRAY)


def _empty_table():
    B = FbBuilder()
    return B.finish_size_prefixed(B.table([]))


# --------------------------------------------------------------------------------------------- writer against reader, model, verifier
CASES = [dict(stripped=False, cache=True), dict(stripped=True, cache=True), dict(stripped=False, cache=False)]


@pytest.mark.parametrize("case", CASES, ids=["full", "stripped", "no_cache"])
def test_bin_bundle_writer_against_reader_model_and_verifier(case):
    blobs = BLOBS if case["cache"] else []
    buf = wire.build_bin_bundle(3, MOD, BINS, POLYNS if case["cache"] else [], blobs, **case)
    mdl = model_bin_bundle(3, MOD, BINS, POLYNS, blobs, **case)
    got, want = wire.parse_bin_bundle(buf), wire.parse_bin_bundle(mdl)
    want["consumed"] = got["consumed"] = None                          # the two layouts differ in padding, the fields do not
    assert got == want
    assert got["bundle_idx"] == 3 and got["mod"] == MOD and got["stripped"] == case["stripped"] and got["has_cache"] == case["cache"]
    assert got["item_bins"] == ([] if case["stripped"] else BINS)
    assert got["matching_polyns"] == (POLYNS if case["cache"] and not case["stripped"] else [])
    assert got["coeffs"] == blobs and got["label_bins"] == 0
    assert (got["felt_interp_polyns"], got["batched_interp_polyns"]) == ((0, 0) if case["cache"] else (None, None))
    info = wire.bin_bundle_info(buf)
    assert info["consumed"] == len(buf) and info["n_bins"] == (0 if case["stripped"] else len(BINS)) and info["cache_coeffs"] == len(blobs)
    assert info["largest_bin"] == (0 if case["stripped"] else 8)
    required = {"item_bins", "rows"} | ({"felt_matching_polyns", "batched_matching_polyn", "coeffs"} if case["cache"] else set())
    if not case["stripped"]:
        required |= {"felts"}
    if case["cache"]:
        required |= {"data"}
    for b in (buf, mdl):
        assert required <= verify(b, BIN_BUNDLE)


def test_bundle_idx_zero_a_wide_modulus_and_no_rows():
    t60 = (1 << 60) - 93
    buf = wire.build_bin_bundle(0, t60, [[t60 - 1], []], [[1, 1], [1]], [b"", b"x"])
    got = wire.parse_bin_bundle(buf)
    assert (got["bundle_idx"], got["mod"], got["item_bins"], got["matching_polyns"], got["coeffs"]) == (0, t60, [[t60 - 1], []], [[1, 1], [1]], [b"", b"x"])
    verify(buf, BIN_BUNDLE)
    empty = wire.build_bin_bundle(1, MOD, [], [], [b"pt"])
    assert wire.parse_bin_bundle(empty)["item_bins"] == [] and "rows" in verify(empty, BIN_BUNDLE)
    with pytest.raises(ValueError, match="stripped"):
        wire.build_bin_bundle(1, MOD, [], [], [], stripped=True, cache=False)


def test_three_bundles_one_behind_the_other():
    bufs = [wire.build_bin_bundle(i, MOD, BINS[:i + 2], POLYNS[:i + 2], BLOBS[:i + 1], stripped=(i == 1), cache=(i != 2)) for i in range(3)]
    blob, at = b"".join(bufs), 0
    for i, b in enumerate(bufs):
        info = wire.bin_bundle_info(blob[at:])
        assert info["bundle_idx"] == i and info["consumed"] == len(b)
        assert wire.parse_bin_bundle(blob[at:]) == wire.parse_bin_bundle(b)
        at += info["consumed"]
    assert at == len(blob)


@pytest.mark.parametrize("stripped, compressed, n_hashed, count", [(False, False, 7, 4), (False, True, 7, 0), (True, False, 0, 4)])
def test_header_writer_against_reader_model_and_verifier(stripped, compressed, n_hashed, count):
    params = wire.psu_params_save(common.toy_json())
    key = bytes(3 * i % 256 for i in range(32))
    hashed = [(11 * i + 1, 2**63 + i) for i in range(n_hashed)]
    buf = wire.build_receiver_db_header(params, item_count=123, bin_bundle_count=count, compressed=compressed, stripped=stripped, oprf_key=key,
                                        hashed_items=hashed, nonce_byte_count=16)
    mdl = model_header(params, key, hashed, 123, count, compressed, stripped, nonce=16)
    got, want = wire.parse_receiver_db_header(buf), wire.parse_receiver_db_header(mdl)
    assert got["consumed"] == len(buf) and want["consumed"] == len(mdl)
    got["consumed"] = want["consumed"] = None
    assert got == want
    assert (got["psu_params"], got["oprf_key"], got["hashed_items"]) == (params, key, hashed)
    assert (got["item_count"], got["bin_bundle_count"], got["compressed"], got["stripped"], got["label_byte_count"], got["nonce_byte_count"]) == \
           (123, count, compressed, stripped, 0, 16)
    for b in (buf, mdl):
        assert {"params", "info", "oprf_key", "hashed_items"} <= verify(b, RECEIVER_DB)
    # the header, then BinBundles: the walk of seal.load_reference_db
    bb = wire.build_bin_bundle(1, MOD, BINS, POLYNS, BLOBS)
    assert wire.bin_bundle_info((buf + bb)[wire.receiver_db_header(buf + bb)["consumed"]:])["bundle_idx"] == 1


def test_the_size_bound():
    wire.saved_size_check(2**31 - 1)
    wire.saved_size_check(0)
    for too_big in (2**31, 2**31 + 1, 2**40):
        with pytest.raises(ValueError, match=str(too_big)):
            wire.saved_size_check(too_big)


# --------------------------------------------------------------------------------------------- k_bins_rows on the CPU
@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


def decoded_array(n, degree, counts, seed):
    """poly[d][s] as decode_bundle leaves it: nonzero below the count, 1 at the count, 0 above; a slot that is no bin is all zero"""
    rng = np.random.default_rng(seed)
    poly = np.zeros((degree + 1, n), dtype=np.uint64)
    for s, c in enumerate(counts):
        if c == NONE:
            continue
        poly[:c, s] = rng.integers(1, MOD, size=c, dtype=np.uint64)
        poly[c, s] = 1
    return poly


def run_rows(emu, poly, bins):
    n = poly.shape[1]
    counts = np.zeros(n, dtype=np.uint32)
    emu.emu_bin_counts(vp(poly), C.c_uint64(n), C.c_uint32(poly.shape[0]), vp(counts))
    total = sum(int(c) + 1 for c in counts[:bins])
    out = np.full(total + 4, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    off = np.zeros(bins + 1, dtype=np.uint64)
    rc = emu.emu_bins_rows(vp(poly), C.c_uint64(n), C.c_uint32(poly.shape[0]), vp(counts), C.c_uint32(bins), vp(off), vp(out))
    return rc, counts, off, out, total


@pytest.mark.parametrize("n, degree, bins, which", [(64, 10, 60, "ragged"), (256, 130, 256, "edges")])
def test_emu_bins_rows_against_numpy(emu, n, degree, bins, which):
    if which == "ragged":                                              # counts 0 .. 10 ragged over 60 bins, slots 60 .. 63 are not bins
        counts = [(7 * s + 3) % 11 for s in range(60)] + [NONE] * 4
        assert set(counts[:60]) == set(range(11))
    else:                                                              # every tile edge, in slots and in degrees
        edge = [0, 1, 63, 64, 65, 127, 128, 130]
        counts = [edge[(s + 7) % 8] for s in range(n)]
        for s, c in zip((0, 63, 64, 127, 128, 255), (130, 128, 65, 64, 63, 127)):
            counts[s] = c
        assert set(counts) == set(edge)
    poly = decoded_array(n, degree, counts, seed=n)
    before = poly.copy()
    rc, got_counts, off, out, total = run_rows(emu, poly, bins)
    assert rc == total, emu.emu_last_error()
    assert [int(c) for c in got_counts] == counts
    want_off = np.concatenate(([0], np.cumsum([c + 1 for c in counts[:bins]]))).astype(np.uint64)
    assert (off == want_off).all()
    want = np.concatenate([poly[:counts[s] + 1, s] for s in range(bins)])
    assert (out[:total] == want).all()
    assert (out[total:] == 0xDEADBEEFDEADBEEF).all()                   # the word behind off[bins] stays as it was
    assert (poly == before).all()
    for s in range(bins):                                              # every row is monic, an empty bin is [1]
        assert out[int(off[s + 1]) - 1] == 1


def test_emu_bins_rows_refuses_an_unused_slot_among_the_bins(emu):
    counts = [2, 0, NONE, 1] + [0] * 60
    poly = decoded_array(64, 3, counts, seed=1)
    rc, _, _, out, _ = run_rows(emu, poly, 3)
    assert rc == -1 and b"bin 2" in emu.emu_last_error()
    assert (out == 0xDEADBEEFDEADBEEF).all()
    rc, _, off, out, _ = run_rows(emu, poly, 2)                        # ... which is no concern when it is not one of the bins
    assert rc == 4 and [int(v) for v in out[:4]] == [int(poly[0, 0]), int(poly[1, 0]), 1, 1]


# --------------------------------------------------------------------------------------------- sanitizers: a stand-alone program
def test_saved_writer_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "saved_writer_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", SRC, os.path.join(ROOT, "tests", "native", "saved_writer_harness.cpp"), os.path.join(SRC, "wire.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert r.stdout.strip().endswith("ok")
