"""CPU tier: the constant blocks a context uploads (apsu_amd/csrc/dev_consts.h: build_device_constants), read through the emulation
library.  Three nets:
  * the bytes are the parent commit's (tests/golden/dev_consts_parent.json: one SHA-256 per block and context);
  * the values are right: every derived field recomputed with Python integers from the definitions in dev_consts.h's comments;
  * make_ntt_table gives what its five former call sites computed, and read_switches reads the documented environment."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import common
import edge_values as ev
import emu_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "dev_consts_parent.json")))
ALL_PARAM_FILES = sorted(f[:-5] for f in os.listdir(common.PARAM_DIR) if f.endswith(".json"))
RAW = 1 << 30
MT = 1 << 32


@pytest.fixture(scope="module")
def emu():
    lib = emu_lib.load()
    lib.emu_device_constants.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_int, C.c_uint64, C.c_int, C.c_char_p, C.c_void_p, C.c_uint64]
    lib.emu_ntt_table.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_void_p]
    return lib


def layouts(emu):
    """numpy mirrors of NttTable / DevLevel / DevKey (C layout), checked against the library's sizeof"""
    out = np.zeros(5, dtype=np.uint64)
    emu.emu_dev_layout(out.ctypes.data_as(C.c_void_p))
    nt, lv, ky, ML, MB = (int(v) for v in out)
    ME = ML + MB
    mod = np.dtype([("q", "<u8"), ("r0", "<u8"), ("r1", "<u8")], align=True)
    sh = np.dtype([("w", "<u8"), ("wq", "<u8")], align=True)
    tab = np.dtype([("q", "<u8"), ("ninv", "<u8"), ("ninv_q", "<u8"), ("r1", "<u8"), ("fwd", "<u8"), ("dit", "<u8"), ("scale", "<u8"),
                    ("narrow", "<i4"), ("fold_k", "<u4"), ("fold_c", "<u4"), ("wide_d4", "<u4"), ("r0", "<u8")], align=True)
    level = np.dtype([
        ("L", "<i4"), ("nB", "<i4"), ("nBsk", "<i4"), ("E", "<i4"), ("q", mod, ML), ("bsk", mod, MB), ("ext", mod, ME), ("t", "<u8"),
        ("mac_shift", "<u4", ML), ("mac_chunk", "<u4", ML), ("mac_chunk_k", "<u4", ML), ("mac_bits", "<u4", ML), ("mac_row_off", "<u4", ML),
        ("mac_mask_hi", "<u4", ML), ("coeff_div_plain", "<u8", ML), ("q_mod_t", "<u8"), ("threshold", "<u8"), ("incr", "<u8", ML),
        ("half", "<u8"), ("half_mod", "<u8", ML), ("inv_q_last", sh, ML), ("ext_scale", sh, ML), ("q_to_bsk", "<u8", (MB, ML)),
        ("q_to_mt", "<u4", ML), ("neg_inv_q_mt", "<u4"), ("prod_q_bsk", "<u8", MB), ("inv_mt_bsk", sh, MB), ("t_inv_punct_q", sh, ML),
        ("t_bsk", sh, MB), ("inv_prod_q_bsk", sh, MB), ("inv_punct_B", sh, MB), ("B_to_q", "<u8", (ML, MB)), ("B_to_msk", "<u8", MB),
        ("inv_prod_B_msk", sh), ("prod_B_q", "<u8", ML), ("neg_prod_B_q", "<u8", ML), ("msk_half", "<u8"), ("s_q_to_bsk", sh, (MB, ML)),
        ("s_prod_q_bsk", sh, MB), ("s_q_to_bsk_mt", sh, (MB, ML)), ("s_prod_q_bsk_mt", sh, MB), ("s_fl", sh, MB), ("s_B_to_q", sh, (ML, MB)),
        ("s_B_to_msk", sh, MB), ("s_prod_B_q", sh, ML), ("s_neg_prod_B_q", sh, ML), ("fin_q", "<u8", ML), ("fin_b", "<u8", MB),
        ("drop_tw", "<u8", ML), ("last_tw", "<u8")], align=True)
    key = np.dtype([("K", "<i4"), ("q", mod, ML + 1), ("p_half", "<u8"), ("p_half_mod", "<u8", ML), ("inv_p", sh, ML), ("md_tw", "<u8", ML),
                    ("p_tw", "<u8")], align=True)
    assert (tab.itemsize, level.itemsize, key.itemsize) == (nt, lv, ky)
    return dict(tab=tab, level=level, key=key, sh=sh, ML=ML, MB=MB, ME=ME)


def block(emu, ctx, name):
    js = common.param_json(ctx["params"]).encode() if "params" in ctx else None
    pr = np.array(ctx.get("primes", []), dtype=np.uint64)
    args = (js, ctx.get("n", 0), pr.ctypes.data, len(pr), ctx.get("t", 0), int(ctx["aux"] == "narrow"), name.encode())
    size = emu.emu_device_constants(*args, None, 0)
    assert size >= 0, emu.emu_last_error()
    buf = np.zeros(size, dtype=np.uint8)
    assert emu.emu_device_constants(*args, buf.ctypes.data, size) == size
    return buf


class Blocks:
    def __init__(self, emu, ctx):
        self.raw = {b: block(emu, ctx, b) for b in GOLDEN["blocks"]}
        ly = self.ly = layouts(emu)
        self.tabs = self.raw["tabs"].view(ly["tab"])
        self.levels = self.raw["levels"].view(ly["level"])
        self.key = self.raw["key"].view(ly["key"])[0]
        self.tw, self.fin, self.drop, self.mdtw = (self.raw[b].view(ly["sh"]) for b in ("tw", "fin", "drop", "mdtw"))
        self.maps = {b: self.raw[b].view("<i4") for b in GOLDEN["blocks"] if b.startswith("map_")}
        self.scalars = [int(v) for v in self.raw["scalars"].view("<u8")]
        self.K = int(self.key["K"])
        self.keyq = [int(self.key["q"][j]["q"]) for j in range(self.K)]


@pytest.fixture(scope="module")
def golden_blocks(emu):
    return {c["name"]: Blocks(emu, c) for c in GOLDEN["contexts"]}


# ------------------------------------------------------------------------------------------------ same bytes as the parent
def test_golden_covers_the_contexts_the_proof_needs():
    names = {c["name"]: c for c in GOLDEN["contexts"]}
    assert {"16M-4096", "256M-4096", "1M-1024-com", "1M-1", "16M-4096-seal", "n32768"} <= set(names)
    assert names["16M-4096-seal"]["aux"] == "seal" and names["n32768"]["n"] == 32768 and len(names["n32768"]["primes"]) == 3
    assert all(50 <= int(q).bit_length() <= 60 for q in names["n32768"]["primes"])
    assert json.loads(common.param_json(names["1M-1"]["params"]))["seal_params"]["coeff_modulus_bits"] == [48]


@pytest.mark.parametrize("ctx", GOLDEN["contexts"], ids=lambda c: c["name"])
def test_blocks_are_the_parents_bytes(golden_blocks, ctx):
    got = golden_blocks[ctx["name"]].raw
    for b in GOLDEN["blocks"]:
        assert hashlib.sha256(got[b].tobytes()).hexdigest() == ctx["sha256"][b], (ctx["name"], b)


# ------------------------------------------------------------------------------------------------ the values are right
def shoup_ok(m, s):
    """a ShoupConst of modulus m: returns w after checking wq = floor(w 2^64 / m)"""
    w, wq = int(s["w"]), int(s["wq"])
    assert w < m and wq == (w << 64) // m, (m, w, wq)
    return w


def prod(v):
    r = 1
    for x in v:
        r *= x
    return r


def check_context(emu, B, n, t, full_tables):
    """every derived field of the blocks B of a context with ring size n and plain modulus t"""
    ly = B.ly
    K, keyq = B.K, B.keyq
    split = n == 32768
    nmod = len(B.tabs) // (2 if split else 1)
    ks = K > 1
    scale = lambda m: B.tw[(m * 3 + 2) * n:(m * 3 + 3) * n]
    modulus = lambda m: int(B.tabs[m * (2 if split else 1)]["q"])
    pos = range(n) if full_tables else sorted({0, 1, 2, n // 2 - 1, n // 2, n - 2, n - 1} | set(range(3, n, 61)))
    # the transforms' own tables: scale[k] = n^-1 psi^-k with psi = fwd[n / 2] a primitive 2n-th root
    ninv_psi = {}
    for m in range(nmod):
        q = modulus(m)
        sc = scale(m)
        ninv = shoup_ok(q, sc[0])
        assert ninv * n % q == 1
        psi = int(B.tw[m * 3 * n + n // 2]["w"])
        assert pow(psi, n, q) == q - 1
        psi_inv = pow(psi, -1, q)
        for k in pos:
            assert shoup_ok(q, sc[k]) == ninv * pow(psi_inv, k, q) % q
        ninv_psi[m] = (ninv, psi_inv)
        for h in range(2 if split else 1):
            tb = B.tabs[m * 2 + h] if split else B.tabs[m]
            assert (int(tb["dit"]), int(tb["scale"])) == (1 + (m * 3 + 1) * n, 1 + (m * 3 + 2) * n)
            assert int(tb["fwd"]) == 1 + (nmod * 3 * n + (m * 2 + h) * (n // 2) if split else m * 3 * n)
            if split:                                                   # W_h[2^s + b] = W[2^(s+1) + h 2^s + b]
                half, fwd = B.tw[int(tb["fwd"]) - 1:int(tb["fwd"]) - 1 + n // 2], B.tw[m * 3 * n:(m * 3 + 1) * n]
                m2 = 1
                while m2 < n // 2:
                    assert (half[m2:2 * m2] == fwd[2 * m2 + h * m2:2 * m2 + h * m2 + m2]).all()
                    m2 *= 2
                assert (int(tb["ninv"]), int(tb["ninv_q"])) == (int(fwd[1]["w"]), int(fwd[1]["wq"]))

    def twisted(table, ref, m, cst):
        """table[ref - 1 ..][k] = cst scale_m[k] mod its modulus, every entry a Shoup pair"""
        assert ref >= 1
        q, (ninv, psi_inv) = modulus(m), ninv_psi[m]
        seg = table[ref - 1:ref - 1 + n]
        assert len(seg) == n
        for k in pos:
            assert shoup_ok(q, seg[k]) == cst * ninv * pow(psi_inv, k, q) % q, (m, k)

    fin_next = drop_next = 1
    for c, d in enumerate(B.levels):
        L, nB = int(d["L"]), int(d["nB"])
        assert (L, int(d["nBsk"]), int(d["E"]), int(d["t"])) == (c + 1, nB + 1, L + nB + 1, t)
        q = keyq[:L]
        bsk = [int(d["bsk"][i]["q"]) for i in range(nB + 1)]
        Bb, msk = bsk[:nB], bsk[nB]
        Q, PB = prod(q), prod(Bb)
        for arr, mods in (("q", q), ("bsk", bsk), ("ext", q + bsk)):
            for i, m in enumerate(mods):
                e = d[arr][i]
                assert int(e["q"]) == m and (int(e["r1"]) << 64 | int(e["r0"])) == (1 << 128) // m
        assert int(d["half"]) == q[-1] >> 1 and int(d["msk_half"]) == msk >> 1 and int(d["q_mod_t"]) == Q % t
        assert int(d["neg_inv_q_mt"]) == -pow(Q, -1, MT) % MT
        for j, qj in enumerate(q):
            punct = Q // qj
            ipq = pow(punct, -1, qj)
            assert shoup_ok(qj, d["ext_scale"][j]) == MT * ipq % qj
            assert shoup_ok(qj, d["t_inv_punct_q"][j]) == t * ipq % qj
            assert int(d["q_to_mt"][j]) == punct % MT
            assert int(d["half_mod"][j]) == (q[-1] >> 1) % qj
            assert int(d["coeff_div_plain"][j]) == (Q // t) % qj and int(d["incr"][j]) == qj - t
            if j + 1 < L:
                assert shoup_ok(qj, d["inv_q_last"][j]) == pow(q[-1], -1, qj)
            else:
                assert (int(d["inv_q_last"][j]["w"]), int(d["inv_q_last"][j]["wq"])) == (0, 0)
            assert int(d["prod_B_q"][j]) == PB % qj == shoup_ok(qj, d["s_prod_B_q"][j])
            assert int(d["neg_prod_B_q"][j]) == -PB % qj == shoup_ok(qj, d["s_neg_prod_B_q"][j])
            for i, b in enumerate(Bb):
                assert int(d["B_to_q"][j][i]) == (PB // b) % qj == shoup_ok(qj, d["s_B_to_q"][j][i])
            # k_mac's split and chunks (edge_values restates them), the packed row geometry
            s = int(d["mac_shift"][j])
            assert (s, int(d["mac_chunk"][j]), int(d["mac_chunk_k"][j])) == (ev.mac_shift(qj), ev.mac_chunk(qj), ev.mac_chunk_kara(qj))
            w = int(d["mac_bits"][j])
            fits = lambda w_: all((2 * w_ * m) % 32 + 2 * w_ <= 128 for m in range(n // 2))    # dev_consts.h: a lane's 16-byte window
            if ks:
                lo = max(qj.bit_length(), 32)
                assert w == next((w_ for w_ in range(lo, 64) if fits(w_)), 64) == B.scalars[3 + j]
            else:
                assert w == 64
            assert int(d["mac_row_off"][j]) == sum(n * int(b) // 8 for b in d["mac_bits"][:j])
            assert int(d["mac_mask_hi"][j]) == (0xFFFFFFFF if w == 64 else (1 << (w - s)) - 1)
        for i, m in enumerate(bsk):
            imt = pow(MT, -1, m)
            for j, qj in enumerate(q):
                assert int(d["q_to_bsk"][i][j]) == (Q // qj) % m == shoup_ok(m, d["s_q_to_bsk"][i][j])
                assert shoup_ok(m, d["s_q_to_bsk_mt"][i][j]) == (Q // qj) * imt % m
            assert int(d["prod_q_bsk"][i]) == Q % m == shoup_ok(m, d["s_prod_q_bsk"][i])
            assert shoup_ok(m, d["s_prod_q_bsk_mt"][i]) == Q * imt % m
            assert shoup_ok(m, d["inv_mt_bsk"][i]) == imt and shoup_ok(m, d["t_bsk"][i]) == t % m
            iq = pow(Q, -1, m)
            assert shoup_ok(m, d["inv_prod_q_bsk"][i]) == iq
            if i < nB:
                ipb = pow(PB // m, -1, m)
                assert shoup_ok(m, d["s_fl"][i]) == iq * ipb % m and shoup_ok(m, d["inv_punct_B"][i]) == ipb
                assert int(d["B_to_msk"][i]) == (PB // m) % msk == shoup_ok(msk, d["s_B_to_msk"][i])
            else:
                assert shoup_ok(m, d["s_fl"][i]) == iq
        assert shoup_ok(msk, d["inv_prod_B_msk"]) == pow(PB, -1, msk)
        # the maps
        me = B.maps["map_ext"][c * ly["ME"]:(c + 1) * ly["ME"]]
        mf = B.maps["map_ext_fin"][c * ly["ME"]:(c + 1) * ly["ME"]]
        ids = [int(v) for v in me[:L + nB + 1]]
        assert ids[:L] == list(range(L)) and [modulus(i) for i in ids] == q + bsk and not me[L + nB + 1:].any()
        fast = bool(emu.emu_behz_unrolled(L, nB))
        assert [int(v) for v in mf] == [int(v) | (RAW if fast and e < L + nB + 1 else 0) for e, v in enumerate(me)]
        mk = B.maps["map_ks"][c * (ly["ML"] + 1) * ly["ML"]:(c + 1) * (ly["ML"] + 1) * ly["ML"]]
        ma = B.maps["map_ksacc"][c * (ly["ML"] + 1):(c + 1) * (ly["ML"] + 1)]
        for I in range(L + 1):
            want = K - 1 if I == L else I                              # the last row is the special prime's
            assert [int(v) for v in mk[I * L:(I + 1) * L]] == [want] * L and int(ma[I]) == want
        assert not mk[(L + 1) * L:].any() and not ma[L + 1:].any()
        # twist-folded tables
        for e in range(ly["ML"] + ly["MB"]):
            ref = int(d["fin_q"][e]) if e < ly["ML"] else int(d["fin_b"][e - ly["ML"]])
            live = fast and (e < L or ly["ML"] <= e < ly["ML"] + nB + 1)
            assert (ref != 0) == live
            if live:
                assert ref == fin_next
                fin_next += n
                j = e if e < L else L + e - ly["ML"]
                twisted(B.fin, ref, ids[j], int(d["t_inv_punct_q"][j]["w"]) if e < L else t % bsk[e - ly["ML"]])
        for j in range(ly["ML"]):
            ref = int(d["drop_tw"][j])
            assert (ref != 0) == (c >= 1 and j + 1 < L)
            if ref:
                assert ref == drop_next
                drop_next += n
                twisted(B.drop, ref, j, pow(q[-1], -1, q[j]))
        assert int(d["last_tw"]) == (1 + ((L - 1) * 3 + 2) * n if c >= 1 else 0)
    assert fin_next - 1 == len(B.fin) and drop_next - 1 == len(B.drop)
    assert (B.maps["map_ksacc_raw"] == (B.maps["map_ksacc"] | RAW)).all()
    assert [int(v) for v in B.maps["map_ct"]] == list(range(ly["ML"] + ly["MB"] + 4))
    # the key block
    k = B.key
    for j in range(ly["ML"] + 1):
        e = k["q"][j]
        assert (int(e["q"]), int(e["r1"]) << 64 | int(e["r0"])) == ((keyq[j], (1 << 128) // keyq[j]) if j < K else (0, 0))
    p = keyq[-1]
    assert int(k["p_half"]) == (p >> 1 if ks else 0) and int(k["p_tw"]) == (1 + ((K - 1) * 3 + 2) * n if ks else 0)
    for j in range(ly["ML"]):
        ref = int(k["md_tw"][j])
        assert (ref != 0) == (ks and j < K - 1)
        if ref:
            assert ref == 1 + j * n and int(k["p_half_mod"][j]) == (p >> 1) % keyq[j]
            assert shoup_ok(keyq[j], k["inv_p"][j]) == pow(p, -1, keyq[j])
            twisted(B.mdtw, ref, j, pow(p, -1, keyq[j]))
    assert len(B.mdtw) == (K - 1) * n if ks else len(B.mdtw) == 0
    # seed expansion's view of the key level, and the scalar facts
    kl = B.raw["key_level"].view(ly["level"])
    first = len(B.levels) - 1
    assert len(kl) == (1 if K - 1 > first else 0)
    if len(kl):
        want = np.zeros(1, dtype=ly["level"])
        want["L"] = K
        want["q"][0][:K] = k["q"][:K]
        assert kl.tobytes() == want.tobytes()
    assert [int(v) for v in B.raw["max_multiple"].view("<u8")] == [(1 << 64) - 1 - ((1 << 64) - 1) % q - 1 for q in keyq]
    logn = n.bit_length() - 1
    narrow = lambda q: q * (4 * logn + 1) < 1 << 64
    aux = [modulus(m) for m in range(K, nmod)]                             # (with the plain modulus' table: far too small to matter)
    assert B.scalars[0] == all(narrow(q) for q in keyq)
    assert B.scalars[1] == (B.scalars[0] and all(narrow(q) for q in aux))
    assert len(B.scalars) == 3 + K


def ctx_n_t(ctx):
    if "params" not in ctx:
        return ctx["n"], ctx["t"]
    from oracle import ref
    Cx = ref.RefContext.from_params(ref.load_params(common.param_json(ctx["params"])))
    return Cx.n, Cx.t


@pytest.mark.parametrize("ctx", GOLDEN["contexts"], ids=lambda c: c["name"])
def test_values_from_their_definitions(emu, golden_blocks, ctx):
    n, t = ctx_n_t(ctx)
    B = golden_blocks[ctx["name"]]
    check_context(emu, B, n, t, full_tables=n <= 8192)
    if "params" in ctx:
        from oracle import ref
        Cx = ref.RefContext.from_params(ref.load_params(common.param_json(ctx["params"])))
        assert B.keyq == Cx.q and B.scalars[2] == int(Cx.q[0] // 2 >= Cx.t and Cx.q[0] > 2 * Cx.t)


@pytest.mark.parametrize("name", ALL_PARAM_FILES)
def test_values_for_every_parameter_file(emu, name):
    """every prime of every shipped file (table positions sampled: the six recorded contexts run every position)"""
    from oracle import ref
    Cx = ref.RefContext.from_params(ref.load_params(common.param_json(name)))
    B = Blocks(emu, {"params": name, "aux": "narrow"})
    assert B.keyq == Cx.q
    check_context(emu, B, Cx.n, Cx.t, full_tables=False)


# ------------------------------------------------------------------------------------------------ make_ntt_table
# primes = 1 mod 2^14 below 2^56, 2^60, 2^61: narrow, wide, and wide next to 2^61 (csub_top_near's) at logn 12 and 13
# (the 61-bit one is the 31st from the top: the first ones are SEAL's auxiliary base, which a coefficient modulus must not meet)
TABLE_PRIMES = {"narrow": 72057594037616641, "wide": 1152921504606830593, "near-wide": 2305843009201242113}


def fold_params(q):
    bits = q.bit_length()
    if bits < 33 or bits > 62:
        return 0, 0
    c = (1 << bits) - q
    if c >> 32 or ((1 << (64 - bits)) + 2) * c > 1 << bits:
        return 0, 0
    return bits, c


def wide_d4(q, narrow):
    if narrow or q >> 61 or 4 * q >= 1 << 63:
        return 0
    d = (1 << 63) - 4 * q
    return 0 if d >> 32 else d


@pytest.mark.parametrize("kind", sorted(TABLE_PRIMES))
@pytest.mark.parametrize("logn", [12, 13])
def test_make_ntt_table_is_what_its_former_call_sites_computed(emu, kind, logn):
    q = TABLE_PRIMES[kind]
    n = 1 << logn
    assert q % (2 * n) == 1
    narrow = int(q * (4 * logn + 1) < 1 << 64)
    fk, fc = fold_params(q)
    d4 = wide_d4(q, narrow)
    assert (narrow, bool(d4)) == {"narrow": (1, False), "wide": (0, False), "near-wide": (0, True)}[kind]
    ninv = pow(n, -1, q)
    r = (1 << 128) // q
    full = dict(q=q, ninv=ninv, ninv_q=(ninv << 64) // q, r1=r >> 64, r0=r & ((1 << 64) - 1), narrow=narrow, fold_k=fk, fold_c=fc, wide_d4=d4)
    names = ["q", "ninv", "ninv_q", "r1", "r0", "narrow", "fold_k", "fold_c", "wide_d4"]
    out = np.zeros(9, dtype=np.uint64)
    # the engine's constructor filled every field; the two transform emulations everything but r0; emu_reduce_any q, r1 and the fold;
    # emu_reduce128 q and the fold; narrow_aux_base's `usable` q, narrow and the fold
    assert emu.emu_ntt_table(q, logn, 1, out.ctypes.data) == 0, emu.emu_last_error()
    got = dict(zip(names, (int(v) for v in out)))
    assert got == full
    assert emu.emu_ntt_table(q, logn, 0, out.ctypes.data) == 0
    got = dict(zip(names, (int(v) for v in out)))
    assert got == dict(full, ninv=0, ninv_q=0)
    for site in (("q", "r1", "fold_k", "fold_c"), ("q", "fold_k", "fold_c"), ("q", "narrow", "fold_k", "fold_c")):
        assert all(got[f] == full[f] for f in site)


# ------------------------------------------------------------------------------------------------ environment switches
SWITCH_FIELDS = ["two_stream_default", "eval_side", "packed_rows", "eval_ws_bytes", "arena_bytes", "force_per_term", "mac_kara",
                 "seed_expand_host", "fuse_tail", "ntt_latency_limbs"]
SWITCH_DEFAULTS = dict(two_stream_default=-1, eval_side=1, packed_rows=1, eval_ws_bytes=6 << 30, arena_bytes=-1, force_per_term=0, mac_kara=-1,
                       seed_expand_host=0, fuse_tail=1, ntt_latency_limbs=-1)             # -1 in a size: "by ring size" / the measured crossover
# variable -> field, and the documented values with what they read as (atoi(v) != 0 for the flags)
SWITCHES = {
    "APSU_HE_SPLIT": ("two_stream_default", {"0": 0, "1": 1, "2": 1}),
    "APSU_HE_EVAL_SIDE": ("eval_side", {"0": 0, "1": 1}),
    "APSU_HE_PACKED_ROWS": ("packed_rows", {"0": 0, "1": 1}),
    "APSU_HE_EVAL_WS_BYTES": ("eval_ws_bytes", {"1048576": 1 << 20, "8589934592": 8 << 30}),
    "APSU_HE_ARENA_BYTES": ("arena_bytes", {"0": 0, "4194304": 4 << 20}),
    "APSU_HE_EVAL_PER_TERM": ("force_per_term", {"1": 1, "0": 0}),
    "APSU_HE_MAC_KARA": ("mac_kara", {"0": 0, "1": 1}),
    "APSU_HE_SEED_EXPAND_HOST": ("seed_expand_host", {"1": 1, "0": 0, "": 0}),
    "APSU_HE_FUSE_TAIL": ("fuse_tail", {"0": 0, "1": 1}),
    "APSU_HE_NTT_LATENCY_LIMBS": ("ntt_latency_limbs", {"0": 0, "256": 256}),
}
CHILD = """
import ctypes, json, os, sys
sys.path.insert(0, sys.argv[1])
import emu_lib
lib = emu_lib.load()
name, values = sys.argv[2], json.loads(sys.argv[3])
out = (ctypes.c_int64 * 10)()
res = {}
for v in ([None] if not name else values):
    if v is not None:
        os.environ[name] = v
    lib.emu_switches(out)
    res[str(v)] = list(out)
print(json.dumps(res))
"""


# a switch added after the ten above is read through emu_switches_more (emu_switches keeps writing ten values)
MORE_FIELDS = ["seed_rej_cap"]
MORE_DEFAULTS = dict(seed_rej_cap=8192)
# (read as written; a context refuses a value outside 1 .. 8192 at create: tests/test_gpu_query_steps.py)
MORE_SWITCHES = {"APSU_HE_SEED_REJ_CAP": ("seed_rej_cap", {"1": 1, "16": 16, "8192": 8192, "0": 0, "8193": 8193, "": 0})}
CHILD_MORE = """
import ctypes, json, os, sys
sys.path.insert(0, sys.argv[1])
import emu_lib
lib = emu_lib.load()
name, values = sys.argv[2], json.loads(sys.argv[3])
out, ten = (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 10)()
res = {}
for v in ([None] if not name else values):
    if v is not None:
        os.environ[name] = v
    k = lib.emu_switches_more(out, 4)
    lib.emu_switches(ten)
    res[str(v)] = [list(out)[:k], list(ten)]
print(json.dumps(res))
"""


def test_switches_added_later(emu):
    """APSU_HE_SEED_REJ_CAP: its default, every documented value, and that it moves none of the ten older switches"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("APSU_HE_")}

    def read(name, values):
        r = subprocess.run([sys.executable, "-c", CHILD_MORE, os.path.join(ROOT, "tests"), name, json.dumps(values)], capture_output=True, text=True, env=env, timeout=60)
        assert r.returncode == 0, r.stderr
        return json.loads(r.stdout)

    more, ten = read("", [])["None"]
    assert dict(zip(MORE_FIELDS, more)) == MORE_DEFAULTS and len(more) == len(MORE_FIELDS)
    assert dict(zip(SWITCH_FIELDS, ten)) == SWITCH_DEFAULTS
    for name, (field, values) in MORE_SWITCHES.items():
        got = read(name, list(values))
        for v, want in values.items():
            assert dict(zip(MORE_FIELDS, got[v][0])) == dict(MORE_DEFAULTS, **{field: want}), (name, v)
            assert dict(zip(SWITCH_FIELDS, got[v][1])) == SWITCH_DEFAULTS, (name, v)


def read_in_child(name, values):
    env = {k: v for k, v in os.environ.items() if not k.startswith("APSU_HE_")}
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(ROOT, "tests"), name, json.dumps(values)], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, r.stderr
    return {k: dict(zip(SWITCH_FIELDS, v)) for k, v in json.loads(r.stdout).items()}


def test_switch_defaults(emu):
    assert sorted(f for f, _ in SWITCHES.values()) == sorted(SWITCH_FIELDS)
    assert read_in_child("", [])["None"] == SWITCH_DEFAULTS


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_switch_values(emu, name):
    field, values = SWITCHES[name]
    got = read_in_child(name, list(values))
    for v, want in values.items():
        assert got[v] == dict(SWITCH_DEFAULTS, **{field: want}), (name, v)
