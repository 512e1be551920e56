"""ctypes binding of the engine's C ABI (include/apsu_he.h).

Names follow the reference interface this path replaces:
  seal::Evaluator::{transform_to_ntt_inplace, transform_from_ntt_inplace, multiply_plain,
  add_inplace, add_plain_inplace, multiply, square, relinearize_inplace,
  mod_switch_to_next_inplace}            receiver/apsu/receiver_osn.cpp:422-478, bin_bundle.cpp:143-357
  Receiver::ComputePowers                receiver/apsu/receiver_osn.cpp:395-488
  BatchedPlaintextPolyn::eval{,_patstock} receiver/apsu/bin_bundle.cpp:106-174,192-360
Errors: APSU_HE_INVALID_ARGUMENT -> ValueError (std::invalid_argument in the reference),
everything else -> ApsuHeError (std::runtime_error / std::logic_error).
"""
import collections
import ctypes as C
import json
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
u64p = C.POINTER(C.c_uint64)


class ApsuHeError(RuntimeError):
    pass


class _Info(C.Structure):
    _fields_ = [
        ("poly_modulus_degree", C.c_uint64), ("plain_modulus", C.c_uint64),
        ("coeff_modulus_size", C.c_int32), ("first_chain_idx", C.c_int32),
        ("using_keyswitching", C.c_int32), ("irrelevant_bit_count", C.c_int32),
        ("coeff_modulus", C.c_uint64 * 8),
        ("ps_low_degree", C.c_uint32), ("max_items_per_bin", C.c_uint32),
        ("bundle_idx_count", C.c_uint32), ("items_per_bundle", C.c_uint32),
        ("source_power_count", C.c_uint32), ("target_power_count", C.c_uint32),
        ("powers_dag_depth", C.c_uint32), ("result_polys", C.c_uint32),
    ]


def lib_path():
    return os.path.join(_HERE, "libapsu_he_gpu.so")


def _preload_shared_hip_runtime():
    """One process must hold ONE HIP runtime.  The PyTorch-ROCm wheel bundles its own libamdhip64
    (same SONAME as /opt/rocm's); whichever is loaded first wins.  If this library came first, a later
    `import torch` would bring a second runtime that sees no GPU ("No HIP GPUs are available"), and
    device pointers could not be shared with torch tensors.  So when torch is installed but not yet
    imported, load torch's copy first; the engine then binds to it through the SONAME."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library():
    """Loads libapsu_he_gpu.so; raises (never falls back) if it has not been built."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise ApsuHeError(
                "HIP extension %s is missing: build it with `make -C apsu_amd/csrc` "
                "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback" % path)
        _preload_shared_hip_runtime()
        _LIB = C.CDLL(path)
        _LIB.apsu_he_last_error.restype = C.c_char_p
    return _LIB


def _check(rc):
    if rc == 0:
        return
    msg = load_library().apsu_he_last_error().decode("utf-8", "replace")
    if rc == -1:
        raise ValueError(msg)
    raise ApsuHeError("apsu_he status %d: %s" % (rc, msg))


def _p(a):
    assert isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"], "need contiguous uint64"
    return a.ctypes.data_as(u64p)


def _ptr_array(items):
    """items: numpy arrays (host) or ints (device pointers) -> (const uint64_t* const*)"""
    arr = (C.c_void_p * len(items))()
    for i, it in enumerate(items):
        arr[i] = it.ctypes.data if isinstance(it, np.ndarray) else int(it)
    return arr


def _update_lists(inserts, removes):
    """per-bin lists -> the six list arguments of apsu_he_bundle_update (+ the arrays that back them, + bins)"""
    nb = max(len(inserts or []), len(removes or []))
    args, keep = [], []
    for lists in (inserts, removes):
        if lists is None:
            args += [None, None, 0]
            continue
        stride = max([len(b) for b in lists] + [1])
        roots = np.zeros((max(nb, 1), stride), dtype=np.uint64)
        counts = np.zeros(max(nb, 1), dtype=np.uint32)
        for i, b in enumerate(lists):
            counts[i] = len(b)
            roots[i, :len(b)] = b
        keep += [roots, counts]
        args += [_p(roots), C.c_void_p(counts.ctypes.data), stride]
    return args, keep, nb


def _entries(entries, felts_per_item):
    """entries: (felts [count][F], start_bins [count]) arrays, or a sequence of (start_bin, felts) pairs -> contiguous (uint64, uint32) arrays"""
    if isinstance(entries, tuple) and len(entries) == 2 and isinstance(entries[0], np.ndarray) and entries[0].ndim == 2:
        felts, start = entries
    else:
        entries = list(entries if entries is not None else [])
        felts = [[int(v) for v in f] for _, f in entries]
        start = [int(s) for s, _ in entries]
    felts = np.ascontiguousarray(felts, dtype=np.uint64).reshape(-1, felts_per_item)
    start = np.ascontiguousarray(start, dtype=np.uint32).reshape(-1)
    if len(felts) != len(start):
        raise ValueError("entries: felts and start bins differ in length")
    return felts, start


NOT_A_BIN = 0xFFFFFFFF


def _bins_stride(counts):
    held = counts[counts != NOT_A_BIN]
    return max(int(held.max()) if held.size else 0, 1)


def _bins_list(roots, counts):
    return [None if c == NOT_A_BIN else roots[s, :int(c)].copy() for s, c in enumerate(counts)]
ENTRY_INSERTED, ENTRY_DUPLICATE, ENTRY_REMOVED, ENTRY_NOT_FOUND = 0, 1, 2, 3
BUNDLE_UNCHANGED, BUNDLE_REPLACED, BUNDLE_EMPTY = 0, 1, 2
ApplyResult = collections.namedtuple("ApplyResult", "state bundles appended ins_status ins_target rem_status rem_target")
CompactResult = collections.namedtuple("CompactResult", "group merged")
BundleInfo = collections.namedtuple("BundleInfo", "slot bundle_idx cache_idx degree")
MultiApplyResult = collections.namedtuple("MultiApplyResult", "new_id n_appended ins_status ins_target rem_status rem_target")


class _SelfTestReport(C.Structure):
    _fields_ = [("bundles", C.c_uint32), ("reserved", C.c_uint32), ("slots", C.c_uint64), ("mismatches", C.c_uint64),
                ("first_bundle", C.c_int32), ("first_slot", C.c_uint32), ("first_got", C.c_uint64), ("first_expected", C.c_uint64),
                ("min_budget_bits", C.c_int32), ("min_budget_bundle", C.c_int32), ("he_ms", C.c_double), ("plain_ms", C.c_double)]


SelfTestReport = collections.namedtuple("SelfTestReport", "bundles slots mismatches first_mismatch min_budget min_budget_bundle he_ms plain_ms")


class _StepArgs(C.Structure):          # apsu_he_step_args
    _fields_ = [("step", C.c_int32), ("chain_idx", C.c_int32), ("flags", C.c_uint32), ("terms", C.c_int32), ("polys", C.c_int32),
                ("batch", C.c_int32), ("e0", C.c_int32), ("n_ext", C.c_int32), ("inp", u64p * 6), ("in_words", C.c_size_t * 6),
                ("out", u64p * 2), ("out_words", C.c_size_t * 2)]


# apsu_he_debug_run_step: the step ids (APSU_HE_STEP_*) by name, and the flags
STEPS = {name: i for i, name in enumerate((
    "level_info", "behz_ext", "drop_behz_ext", "tensor", "tensor_conv", "tensor_sum", "behz_finish", "behz_finish_sum", "ks_inner",
    "ks_moddown", "modswitch", "modswitch_jobs", "i0_finish", "eval_epilogue", "add_many", "sum_jobs", "add_plain", "dyadic_plain", "lift",
    "polyn_with_roots", "bins_update", "bin_counts", "poly_degree", "bins_lookup", "bins_merge", "bins_rows", "bins_eval", "eval_compare", "roots",
    "unlift", "ntt_info", "ntt", "ntt_gather", "intt_tensor", "roots_split",
    "seed_expand", "decrypt_round", "plain_powers", "sample_small", "small_lift", "enc_finish", "rlk_finish", "flag_monomial",
    "mac_info", "mac", "term_product", "pack_rows", "unpack_rows", "limb0_rows", "entries_scatter",
    "bucket_count", "bucket_keys", "bucket_scan", "bucket_hist", "bucket_scatter", "bucket_offsets", "bucket_order", "entries_gather",
    "add", "clear_bits", "copy_jobs", "copy_sources", "fill_random", "fill_blake2xb", "scatter_slots", "gather_slots", "algebraize", "pack_blocks"))}
STEP_RAW, STEP_ACCUMULATE, STEP_STORE, STEP_KEY, STEP_PLAN, STEP_COMPOSED, STEP_INVERSE, STEP_NORED = 1, 2, 4, 8, 16, 32, 64, 128
STEP_KARA, STEP_PACKED, STEP_LIMB_SLOW = 256, 512, 1024      # the multiply-accumulate steps: three products, bit-packed plaintexts, grid order
STEP_MAP_RAW = 1 << 30                 # in a map entry of an inverse transform step: that limb comes back RAW


def _self_test_report(r):
    """first_mismatch: None, or (BinBundle, slot, got, expected); min_budget_bundle: None when nothing was checked"""
    first = None if r.first_bundle < 0 else (int(r.first_bundle), int(r.first_slot), int(r.first_got), int(r.first_expected))
    return SelfTestReport(int(r.bundles), int(r.slots), int(r.mismatches), first, int(r.min_budget_bits),
                          None if r.min_budget_bundle < 0 else int(r.min_budget_bundle), float(r.he_ms), float(r.plain_ms))


class RelinKeys:
    def __init__(self, ctx, handle):
        self._ctx, self.h = ctx, handle

    def __del__(self):
        try:
            if self.h:
                load_library().apsu_he_relin_free(self.h)
        except Exception:
            pass


class Bundle:
    """Device-resident BinBundleCache.batched_matching_polyn (receiver/apsu/bin_bundle.h:52-134)."""

    def __init__(self, ctx, handle, bundle_idx, cache_idx, degree):
        self._ctx, self.h = ctx, handle
        self.bundle_idx, self.cache_idx, self.degree = bundle_idx, cache_idx, degree

    @property
    def db_bytes(self):
        v = C.c_uint64()
        _check(load_library().apsu_he_bundle_bytes(self.h, C.byref(v)))
        return v.value

    def __del__(self):
        try:
            if self.h:
                load_library().apsu_he_bundle_free(self.h)
        except Exception:
            pass


class Powers:
    """Device-resident CiphertextPowers (receiver/apsu/receiver_osn.h:41) for some bundle indices."""

    def __init__(self, ctx, handle, bundle_indices):
        self._ctx, self.h, self.bundle_indices = ctx, handle, list(bundle_indices)

    def download(self, bundle_idx, power):
        """-> (ct [size][L][n], chain_idx, is_ntt) in the form receiver_osn.cpp:459-487 leaves it (size 2 with key switching)."""
        ctx = self._ctx
        sz = ctx.power_size(power)
        buf = np.empty(sz * (ctx.first_chain_idx + 1) * ctx.n, dtype=np.uint64)
        ci, ntt = C.c_int(), C.c_int()
        _check(load_library().apsu_he_powers_download(ctx.h, self.h, bundle_idx, power, _p(buf), C.c_size_t(buf.size),
                                                     C.byref(ci), C.byref(ntt)))
        L = ci.value + 1
        return buf[: sz * L * ctx.n].reshape(sz, L, ctx.n).copy(), ci.value, bool(ntt.value)

    def __del__(self):
        try:
            if self.h:
                load_library().apsu_he_powers_free(self.h)
        except Exception:
            pass


class HeContext:
    """CryptoContext + seal::Evaluator replacement (common/apsu/crypto_context.h:28-125)."""

    def __init__(self, psu_params_json=None, device=0, n=None, coeff_modulus=None, plain_modulus=None):
        L = load_library()
        h = C.c_void_p()
        if psu_params_json is not None:
            if os.path.exists(psu_params_json):
                with open(psu_params_json) as f:
                    psu_params_json = f.read()
            _check(L.apsu_he_create(psu_params_json.encode(), device, C.byref(h)))
            js = json.loads(psu_params_json)
            self.felts_per_item = int(js["item_params"]["felts_per_item"])
            self.table_size = int(js["table_params"]["table_size"])
            self.hash_func_count = int(js["table_params"]["hash_func_count"])
        else:
            self.felts_per_item = self.table_size = self.hash_func_count = 0
            q = np.array(coeff_modulus, dtype=np.uint64)
            _check(L.apsu_he_create_raw(C.c_uint64(n), _p(q), len(q), C.c_uint64(plain_modulus), device, C.byref(h)))
        self.h = h
        self.device = int(device)
        info = _Info()
        _check(L.apsu_he_get_info(self.h, C.byref(info)))
        self.info = info
        self.n = int(info.poly_modulus_degree)
        self.t = int(info.plain_modulus)
        self.K = int(info.coeff_modulus_size)
        self.first_chain_idx = int(info.first_chain_idx)
        self.q = [int(info.coeff_modulus[i]) for i in range(self.K)]
        self.ps_low_degree = int(info.ps_low_degree)
        self.max_items_per_bin = int(info.max_items_per_bin)
        self.bundle_idx_count = int(info.bundle_idx_count)
        self.source_power_count = int(info.source_power_count)
        self.irrelevant_bit_count = int(info.irrelevant_bit_count)
        self.result_polys = int(info.result_polys) or 2

    def close(self):
        if getattr(self, "h", None):
            load_library().apsu_he_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def powers_dag(self):
        cnt = C.c_int()
        L = load_library()
        _check(L.apsu_he_get_powers_dag(self.h, None, 0, C.byref(cnt)))
        nodes = np.zeros((cnt.value, 4), dtype=np.uint32)
        _check(L.apsu_he_get_powers_dag(self.h, C.c_void_p(nodes.ctypes.data), cnt.value, C.byref(cnt)))
        return [tuple(int(v) for v in r) for r in nodes]

    PROFILE_CLASSES = ("ntt_fwd", "ntt_inv", "dyadic_mac", "behz_ext", "behz_tensor", "behz_finish", "keyswitch",
                       "modswitch", "other", "ntt_fused")

    def phase_enable(self, on=True):
        """phase timers under the reference's STOPWATCH names (apsu_he_phase_*)"""
        _check(load_library().apsu_he_phase_enable(self.h, 1 if on else 0))

    def phase_read(self, reset=True):
        """-> {"Receiver::RunQuery": (count, avg_ms, min_ms, max_ms), "Receiver::ComputePowers": ..., "Receiver::ProcessBinBundleCache": ...}"""
        L = load_library()
        L.apsu_he_phase_name.restype = C.c_char_p
        out = {}
        for ph in range(3):
            cnt = C.c_uint64(); avg = C.c_double(); mn = C.c_double(); mx = C.c_double()
            _check(L.apsu_he_phase_read(self.h, ph, C.byref(cnt), C.byref(avg), C.byref(mn), C.byref(mx), 0))
            out[L.apsu_he_phase_name(ph).decode()] = (int(cnt.value), avg.value, mn.value, mx.value)
        if reset:
            _check(L.apsu_he_phase_read(self.h, 0, None, None, None, None, 1))
        return out

    def seed_expand(self, chain_idx, seeds, dst_ptrs):
        """apsu_he_seed_expand: seeds [count][8] uint64, dst_ptrs: device pointers ([L][n] words each)"""
        sd = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(-1, 8)
        _check(load_library().apsu_he_seed_expand(self.h, int(chain_idx), len(sd), _p(sd.reshape(-1)), _ptr_array([int(p) for p in dst_ptrs])))

    def compute_powers_cost(self):
        """ComputePowers for one bundle index in the partition rule's cost unit (apsu_he_compute_powers_cost)"""
        v = C.c_uint64()
        _check(load_library().apsu_he_compute_powers_cost(self.h, C.byref(v)))
        return int(v.value)

    COUNTERS = ("host_sync", "job_upload", "job_hit", "arena_grow", "powers_alloc", "stage_wrap", "job_realloc", "pipelined")

    def debug_counters(self):
        """host-side events inside the engine (monotonic): see apsu_he_debug_counters"""
        out = (C.c_uint64 * len(self.COUNTERS))()
        _check(load_library().apsu_he_debug_counters(self.h, out, len(self.COUNTERS)))
        return {k: int(out[i]) for i, k in enumerate(self.COUNTERS)}

    def profile_enable(self, mode=1):
        """0/False off, 1/True every kernel class, 2 NTT launches only (least intrusive)"""
        _check(load_library().apsu_he_profile_enable(self.h, int(mode)))

    def profile_read(self, reset=True):
        """-> {class: (ms, launches, units)} of device time measured with HIP events on the engine's stream."""
        k = len(self.PROFILE_CLASSES)
        ms = (C.c_double * k)()
        la = (C.c_uint64 * k)()
        un = (C.c_uint64 * k)()
        _check(load_library().apsu_he_profile_read(self.h, ms, la, un, k, 1 if reset else 0))
        return {name: (ms[i], int(la[i]), int(un[i])) for i, name in enumerate(self.PROFILE_CLASSES)}

    # ---- tier 1: Evaluator methods (in place on numpy arrays shaped [polys][L][n])
    def transform_to_ntt_inplace(self, ct, chain_idx):
        _check(load_library().apsu_he_transform_to_ntt(self.h, _p(ct), ct.shape[0], chain_idx))

    def transform_from_ntt_inplace(self, ct, chain_idx):
        _check(load_library().apsu_he_transform_from_ntt(self.h, _p(ct), ct.shape[0], chain_idx))

    def transform_plain_to_ntt(self, pt, chain_idx):
        out = np.empty((chain_idx + 1, self.n), dtype=np.uint64)
        _check(load_library().apsu_he_transform_plain_to_ntt(self.h, _p(pt), C.c_size_t(pt.size), _p(out), chain_idx))
        return out

    def multiply_plain_ntt(self, ct, pt_ntt, chain_idx):
        out = np.empty_like(ct)
        _check(load_library().apsu_he_multiply_plain_ntt(self.h, _p(ct), _p(pt_ntt), _p(out), ct.shape[0], chain_idx))
        return out

    def multiply_plain(self, ct, pt, chain_idx):
        out = np.empty_like(ct)
        _check(load_library().apsu_he_multiply_plain(self.h, _p(ct), _p(pt), C.c_size_t(pt.size), _p(out), ct.shape[0], chain_idx))
        return out

    def add_inplace(self, acc, x, chain_idx):
        _check(load_library().apsu_he_add(self.h, _p(acc), _p(x), acc.shape[0], chain_idx))

    def add_plain_inplace(self, ct, pt, chain_idx):
        _check(load_library().apsu_he_add_plain(self.h, _p(ct), _p(pt), C.c_size_t(pt.size), chain_idx))

    def multiply(self, a, b, chain_idx):
        out = np.empty((3, chain_idx + 1, self.n), dtype=np.uint64)
        _check(load_library().apsu_he_multiply(self.h, _p(a), _p(b), _p(out), chain_idx))
        return out

    def square(self, a, chain_idx):
        out = np.empty((3, chain_idx + 1, self.n), dtype=np.uint64)
        _check(load_library().apsu_he_square(self.h, _p(a), _p(out), chain_idx))
        return out

    def multiply_sized(self, a, b, chain_idx):
        """Evaluator::multiply of ciphertexts that were never relinearised: size_a + size_b - 1 polynomials"""
        out = np.empty((a.shape[0] + b.shape[0] - 1, chain_idx + 1, self.n), dtype=np.uint64)
        _check(load_library().apsu_he_multiply_sized(self.h, _p(a), a.shape[0], _p(b), b.shape[0], _p(out), chain_idx))
        return out

    def power_size(self, power):
        """polynomials of a target power after ComputePowers (2 with key switching)"""
        v = C.c_uint32()
        _check(load_library().apsu_he_power_size(self.h, C.c_uint32(power), C.byref(v)))
        return v.value

    def result_size(self, bundle):
        """polynomials of one BinBundle's result (2 with key switching)"""
        v = C.c_uint32()
        _check(load_library().apsu_he_bundle_result_size(self.h, bundle.h, C.byref(v)))
        return v.value

    def relinearize(self, ct3, rk, chain_idx):
        work = np.ascontiguousarray(ct3.copy())
        _check(load_library().apsu_he_relinearize(self.h, _p(work), rk.h, chain_idx))
        return np.ascontiguousarray(work[:2])

    def mod_switch_to_next(self, ct, chain_idx):
        work = np.ascontiguousarray(ct.copy())
        polys = ct.shape[0]
        _check(load_library().apsu_he_mod_switch_to_next(self.h, _p(work), polys, chain_idx))
        return np.ascontiguousarray(work.reshape(-1)[: polys * chain_idx * self.n].reshape(polys, chain_idx, self.n))

    def clear_irrelevant_bits(self, ct):
        _check(load_library().apsu_he_clear_irrelevant_bits(self.h, _p(ct), ct.shape[0]))

    # ---- tier 2
    def upload_relin_keys(self, rk):
        h = C.c_void_p()
        _check(load_library().apsu_he_relin_upload(self.h, _p(np.ascontiguousarray(rk)), C.byref(h)))
        return RelinKeys(self, h)

    def upload_bundle(self, bundle_idx, cache_idx, coeffs, is_ntt):
        """coeffs: list of uint64 arrays (batched_coeffs as Plaintext.data()); is_ntt: list of bool."""
        h = C.c_void_p()
        flags = (C.c_uint8 * len(coeffs))(*[1 if f else 0 for f in is_ntt])
        keep = [np.ascontiguousarray(c, dtype=np.uint64) for c in coeffs]
        _check(load_library().apsu_he_db_upload_bundle(self.h, bundle_idx, cache_idx, len(keep), _ptr_array(keep), flags,
                                                       C.byref(h)))
        return Bundle(self, h, bundle_idx, cache_idx, len(keep) - 1)

    def build_bundle(self, bundle_idx, cache_idx, bins):
        """BinBundle::regen_cache on the GPU.  bins: list (one per bin / slot) of lists of field elements."""
        nb = len(bins)
        stride = max([len(b) for b in bins] + [1])
        roots = np.zeros((max(nb, 1), stride), dtype=np.uint64)
        counts = np.zeros(max(nb, 1), dtype=np.uint32)
        for i, b in enumerate(bins):
            counts[i] = len(b)
            roots[i, :len(b)] = b
        h = C.c_void_p()
        _check(load_library().apsu_he_db_build_bundle(self.h, bundle_idx, cache_idx, _p(roots), C.c_void_p(counts.ctypes.data),
                                                      nb, stride, C.byref(h)))
        deg = C.c_uint32()
        _check(load_library().apsu_he_bundle_degree(h, C.byref(deg)))
        return Bundle(self, h, bundle_idx, cache_idx, deg.value)

    def update_bundle(self, bundle, inserts=None, removes=None):
        """ReceiverDB::insert_or_assign / remove on the GPU: -> a new Bundle = `bundle` with, per bin, the values of removes[bin]
        taken out and then those of inserts[bin] put in (per-bin lists as in build_bundle; None = nothing of that kind).  `bundle`
        needs no roots behind it and stays valid."""
        args, keep, nb = _update_lists(inserts, removes)
        h = C.c_void_p()
        _check(load_library().apsu_he_bundle_update(self.h, bundle.h, *args, nb, C.byref(h)))
        deg = C.c_uint32()
        _check(load_library().apsu_he_bundle_degree(h, C.byref(deg)))
        return Bundle(self, h, bundle.bundle_idx, bundle.cache_idx, deg.value)

    def bin_counts(self, bundle):
        """-> counts [n] uint32: per slot the index of the highest non-zero coefficient of the bin's polynomial, NOT_A_BIN for the zero
        polynomial (apsu_he_bundle_bin_counts)"""
        counts = np.empty(self.n, dtype=np.uint32)
        _check(load_library().apsu_he_bundle_bin_counts(self.h, bundle.h, C.c_void_p(counts.ctypes.data)))
        return counts

    def bins(self, bundle, _form=0):
        """-> the BinBundle's bins read back from its polynomials: a list of n entries, a sorted np.uint64 array per bin (a value of
        multiplicity m appears m times), None for a slot that is not a bin (apsu_he_bundle_bins).  _form: tests only, names the path
        (1: k_bin_roots, 2: the per-coset composition)."""
        lib = load_library()
        counts = np.empty(self.n, dtype=np.uint32)
        _check(lib.apsu_he_bundle_bin_counts(self.h, bundle.h, C.c_void_p(counts.ctypes.data)))   # the stride to ask with
        stride = _bins_stride(counts)
        roots = np.zeros((self.n, stride), dtype=np.uint64)
        if _form:
            _check(lib.apsu_he_debug_bundle_bins_form(self.h, bundle.h, _p(roots), C.c_void_p(counts.ctypes.data), C.c_uint32(stride), C.c_int(_form)))
        else:
            _check(lib.apsu_he_bundle_bins(self.h, bundle.h, _p(roots), C.c_void_p(counts.ctypes.data), C.c_uint32(stride)))
        return _bins_list(roots, counts)

    def debug_run_step(self, step, chain_idx, ins=(), outs=(), flags=0, terms=0, polys=0, batch=1, e0=0, n_ext=0):
        """tests only: ONE element-wise launch on host arrays (apsu_he_debug_run_step; the layouts are in include/apsu_he.h).  step: a
        name of STEPS; ins: up to six uint64 arrays or None; outs: up to two uint64 arrays, written (and read, where the step adds
        into its output).  A refusal raises ValueError with the library's reason."""
        a = _StepArgs()
        a.step, a.chain_idx, a.flags = STEPS[step], chain_idx, flags
        a.terms, a.polys, a.batch, a.e0, a.n_ext = terms, polys, batch, e0, n_ext
        for i, x in enumerate(ins):
            if x is not None:
                a.inp[i], a.in_words[i] = _p(x), x.size
        for i, x in enumerate(outs):
            if x is not None:
                a.out[i], a.out_words[i] = _p(x), x.size
        _check(load_library().apsu_he_debug_run_step(self.h, C.byref(a)))

    def level_info(self, chain_idx):
        """tests only: the moduli of a chain level as the context holds them -> dict(L, nB, unrolled, K, q, B, m_sk, p, clear_bits)"""
        out = np.zeros(64, dtype=np.uint64)
        self.debug_run_step("level_info", chain_idx, outs=[out])
        v = [int(x) for x in out]
        L, nB = v[0], v[1]
        return dict(L=L, nB=nB, unrolled=bool(v[2]), K=v[3], q=v[4:4 + L], B=v[4 + L:4 + L + nB], m_sk=v[4 + L + nB], p=v[5 + L + nB],
                    clear_bits=v[6 + L + nB])

    def eval_plain(self, bundles, x, masks=None, want_is_bin=False):
        """What resident BinBundles answer in plaintext (apsu_he_bundles_eval_plain): x [len(bundles)][n] slot values below t, masks the
        same shape (slot values, not encoded plaintexts) or None -> out [len(bundles)][n] = P_slot(x) + mask mod t, the value a querier
        decrypts; with want_is_bin also a bool array, False where the slot holds the zero polynomial."""
        count = len(bundles)
        x = np.ascontiguousarray(x, dtype=np.uint64).reshape(count, self.n)
        if masks is not None:
            masks = np.ascontiguousarray(masks, dtype=np.uint64).reshape(count, self.n)
        out = np.empty((count, self.n), dtype=np.uint64)
        is_bin = np.zeros((count, self.n), dtype=np.uint8) if want_is_bin else None
        hs = (C.c_void_p * count)(*[b.h for b in bundles])
        _check(load_library().apsu_he_bundles_eval_plain(self.h, hs, C.c_uint32(count), _p(x), 0, _p(masks) if masks is not None else None, 0,
                                                         _p(out), 0, C.c_void_p(is_bin.ctypes.data) if want_is_bin else None))
        return (out, is_bin.astype(bool)) if want_is_bin else out

    def eval_plain_times(self):
        """-> (decode ms, counts ms, k_bins_eval ms): device time of the last eval_plain call, summed over its BinBundles"""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        _check(load_library().apsu_he_debug_eval_plain_times(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def self_test(self, bundles, seed=None, x=None):
        """One real query against resident BinBundles, wholly on the device, held slot for slot against eval_plain of the same values
        (apsu_he_db_self_test) -> SelfTestReport.  x: [distinct bundle indices, ascending][n] slot values, None to draw them from the
        seed.  Proves that the engine's evaluation, decryption and stored polynomials agree; cannot prove agreement with SEAL."""
        sd = self._seed_words(seed)
        count = len(bundles)
        hs = (C.c_void_p * max(count, 1))(*[b.h for b in bundles])
        if x is not None:
            x = np.ascontiguousarray(x, dtype=np.uint64)
            if x.size != len({b.bundle_idx for b in bundles}) * self.n:
                raise ValueError("x must hold n slot values per distinct bundle index")
        rep = _SelfTestReport()
        _check(load_library().apsu_he_db_self_test(self.h, hs, C.c_uint32(count), _p(sd), _p(x) if x is not None else None, C.byref(rep)))
        return _self_test_report(rep)

    def self_test_times(self):
        """-> (decode, counts, k_bins_eval, comparison, homomorphic part) ms: device time of the last self_test call"""
        ms = (C.c_double * 5)()
        _check(load_library().apsu_he_debug_self_test_times(self.h, ms))
        return tuple(float(v) for v in ms)

    def bins_times(self):
        """-> (decode + counts ms, root search ms, multiplicities + copy-back ms): device time of the last bins call"""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        _check(load_library().apsu_he_debug_bins_times(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def lookup(self, bundles, entries):
        """entries ((felts [count][F], start_bins [count]) or (start_bin, felts) pairs) against resident BinBundles -> (present
        [len(bundles)][count] bool, room [len(bundles)][count] uint32 = multi_insert_dry_run's value or NOT_A_BIN); apsu_he_bundles_lookup"""
        felts, start = _entries(entries, self.felts_per_item)
        present = np.zeros((len(bundles), len(start)), dtype=np.uint8)
        room = np.zeros((len(bundles), len(start)), dtype=np.uint32)
        hs = (C.c_void_p * max(len(bundles), 1))(*[b.h for b in bundles])
        _check(load_library().apsu_he_bundles_lookup(self.h, hs, len(bundles), _p(felts), C.c_void_p(start.ctypes.data), C.c_size_t(len(start)),
                                                     C.c_void_p(present.ctypes.data), C.c_void_p(room.ctypes.data)))
        return present.astype(bool), room

    def lookup_times(self):
        """-> (decode ms, kernels ms): device time of the last bin_counts / lookup / apply_entries call, summed over its BinBundles"""
        a, k = C.c_double(), C.c_double()
        _check(load_library().apsu_he_debug_lookup_times(self.h, C.byref(a), C.byref(k)))
        return a.value, k.value

    def apply_entries(self, bundles, inserts=None, removes=None, bundle_idx=None):
        """ReceiverDB::insert_or_assign / remove for a batch of entries on the BinBundles of one bundle index, given in cache order
        (apsu_he_db_apply_entries) -> ApplyResult: state [len(bundles)] (BUNDLE_*), bundles (the new Bundle where REPLACED, else None),
        appended (new Bundles), and per entry status (ENTRY_*) and target position.  `bundles` stay valid.  bundle_idx is needed only
        when no BinBundle is given."""
        if bundle_idx is None:
            if not bundles:
                raise ValueError("apply_entries: bundle_idx is needed when no BinBundle is given")
            bundle_idx = bundles[0].bundle_idx
        fi, si = _entries(inserts, self.felts_per_item)
        fr, sr = _entries(removes, self.felts_per_item)
        nb = len(bundles)
        hs = (C.c_void_p * max(nb, 1))(*[b.h for b in bundles])
        state = np.zeros(nb, dtype=np.uint32)
        replaced = (C.c_void_p * max(nb, 1))()
        appended = (C.c_void_p * max(len(si), 1))()
        n_app = C.c_uint32()
        out = [np.zeros(len(si), dtype=np.uint32), np.zeros(len(si), dtype=np.uint32), np.zeros(len(sr), dtype=np.uint32), np.zeros(len(sr), dtype=np.uint32)]
        u32 = lambda a: C.c_void_p(a.ctypes.data)
        L = load_library()
        _check(L.apsu_he_db_apply_entries(self.h, C.c_uint32(bundle_idx), hs, nb, _p(fi), u32(si), C.c_size_t(len(si)), _p(fr), u32(sr), C.c_size_t(len(sr)),
                                          u32(state), replaced, appended, C.byref(n_app), *[u32(a) for a in out]))

        def wrap(h, bundle_idx, cache_idx):
            h = C.c_void_p(h)
            deg = C.c_uint32()
            _check(L.apsu_he_bundle_degree(h, C.byref(deg)))
            return Bundle(self, h, bundle_idx, cache_idx, deg.value)
        news = [wrap(replaced[i], b.bundle_idx, b.cache_idx) if replaced[i] else None for i, b in enumerate(bundles)]
        first = bundles[-1].cache_idx + 1 if bundles else 0
        apps = [wrap(appended[k], bundle_idx, first + k) for k in range(n_app.value)]
        return ApplyResult(state, news, apps, *out)

    def merge_bundles(self, bundles, cache_idx=None):
        """two or more BinBundles of one bundle index -> a new Bundle holding, per bin, the union (a multiset) of their bins: the
        product of the bins' polynomials (apsu_he_bundles_merge).  cache_idx: the new BinBundle's, default the first input's.  The
        inputs need no roots behind them and stay valid."""
        if cache_idx is None:
            if not bundles:
                raise ValueError("a merge takes at least two BinBundles")
            cache_idx = bundles[0].cache_idx
        hs = (C.c_void_p * max(len(bundles), 1))(*[b.h for b in bundles])
        h = C.c_void_p()
        _check(load_library().apsu_he_bundles_merge(self.h, hs, len(bundles), C.c_uint32(cache_idx), C.byref(h)))
        deg = C.c_uint32()
        _check(load_library().apsu_he_bundle_degree(h, C.byref(deg)))
        return Bundle(self, h, bundles[0].bundle_idx, cache_idx, deg.value)

    def _wrap_new(self, h, bundle_idx, cache_idx):
        h = C.c_void_p(h)
        deg = C.c_uint32()
        _check(load_library().apsu_he_bundle_degree(h, C.byref(deg)))
        return Bundle(self, h, bundle_idx, cache_idx, deg.value)

    def split_bundle(self, bundle, parts, cache_idx=None):
        """one BinBundle -> `parts` new Bundles, the inverse of merge_bundles: part p holds the positions [p c // parts,
        (p + 1) c // parts) of every bin's sorted list of c items (apsu_he_bundle_split).  cache_idx: one per part, default the
        input's and the numbers behind it.  No root reaches the host; the input stays valid."""
        parts = int(parts)
        ci = None if cache_idx is None else np.ascontiguousarray(cache_idx, dtype=np.uint32)
        if ci is not None and len(ci) != parts:
            raise ValueError("split_bundle: one cache_idx per part")
        hs = (C.c_void_p * max(parts, 1))()
        _check(load_library().apsu_he_bundle_split(self.h, bundle.h, C.c_uint32(max(parts, 0)), C.c_void_p(ci.ctypes.data) if ci is not None else None, hs))
        return [self._wrap_new(hs[p], bundle.bundle_idx, int(ci[p]) if ci is not None else bundle.cache_idx + p) for p in range(parts)]

    def adopt_bundle(self, src_ctx, bundle, cache_idx=None):
        """a BinBundle of src_ctx, whose parameters agree with this context's in ring, plain modulus and table and item geometry, as
        a new Bundle of this context with the same bins (apsu_he_bundle_adopt).  cache_idx: default the input's."""
        cache_idx = bundle.cache_idx if cache_idx is None else int(cache_idx)
        h = C.c_void_p()
        _check(load_library().apsu_he_bundle_adopt(self.h, src_ctx.h, bundle.h, C.c_uint32(cache_idx), C.byref(h)))
        return self._wrap_new(h.value, bundle.bundle_idx, cache_idx)

    def rebase_from(self, src_ctx, bundles):
        """the BinBundles of src_ctx moved to this context, split first where this context's max_items_per_bin asks for it
        (apsu_he_db_rebase) -> (new Bundles, origin): origin[i] is the position in `bundles` that output i came from.  All or nothing."""
        nb = len(bundles)
        cap = sum(b.degree + 1 for b in bundles)
        hs = (C.c_void_p * max(nb, 1))(*[b.h for b in bundles])
        out = (C.c_void_p * max(cap, 1))()
        origin, cache = np.zeros(max(cap, 1), dtype=np.uint32), np.zeros(max(cap, 1), dtype=np.uint32)
        n_out = C.c_uint32()
        _check(load_library().apsu_he_db_rebase(self.h, src_ctx.h, hs, nb, out, C.c_void_p(origin.ctypes.data), C.c_void_p(cache.ctypes.data), C.c_uint32(cap),
                                                C.byref(n_out)))
        m = n_out.value
        return [self._wrap_new(out[i], bundles[origin[i]].bundle_idx, int(cache[i])) for i in range(m)], [int(o) for o in origin[:m]]

    def split_times(self):
        """-> (decode + counts, root search + multiplicities, k_roots_split, the parts' builds) ms: device time of the last split_bundle call"""
        v = [C.c_double() for _ in range(4)]
        _check(load_library().apsu_he_debug_split_times(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def merge_times(self):
        """-> (decode ms, kernel ms, encode ms): device time of the last merge_bundles call"""
        a, k, e = C.c_double(), C.c_double(), C.c_double()
        _check(load_library().apsu_he_debug_merge_times(self.h, C.byref(a), C.byref(k), C.byref(e)))
        return a.value, k.value, e.value

    def compact(self, bundle_idx, bundles):
        """the sparse BinBundles of one bundle index, given in cache order, into as few as the placement rule's bound allows
        (apsu_he_db_compact) -> CompactResult: group [len(bundles)] and merged [groups] (the new Bundle of a group of two or more, with
        its first member's cache_idx; None for a group of one, whose BinBundle stays as it is).  `bundles` stay valid."""
        nb = len(bundles)
        hs = (C.c_void_p * max(nb, 1))(*[b.h for b in bundles])
        group = np.zeros(nb, dtype=np.uint32)
        merged = (C.c_void_p * max(nb, 1))()
        made = C.c_uint32()
        L = load_library()
        _check(L.apsu_he_db_compact(self.h, C.c_uint32(bundle_idx), hs, nb, C.c_void_p(group.ctypes.data), merged, C.byref(made)))
        out = []
        for g in range(int(group.max()) + 1 if nb else 0):
            if not merged[g]:
                out.append(None)
                continue
            h = C.c_void_p(merged[g])
            deg = C.c_uint32()
            _check(L.apsu_he_bundle_degree(h, C.byref(deg)))
            first = next(b for i, b in enumerate(bundles) if group[i] == g)
            out.append(Bundle(self, h, bundle_idx, first.cache_idx, deg.value))
        assert sum(m is not None for m in out) == made.value
        return CompactResult(group, out)

    def algebraize_items(self, items):
        """util::algebraize_item for items [count][16] uint8 -> felts [count][felts_per_item] (db_encoding.cpp:209-256,360-366)"""
        items = np.ascontiguousarray(items, dtype=np.uint8).reshape(-1, 16)
        if not self.felts_per_item:
            raise ApsuHeError("context was created without PSUParams")
        out = np.empty((items.shape[0], self.felts_per_item), dtype=np.uint64)
        _check(load_library().apsu_he_algebraize_items(self.h, items.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_size_t(items.shape[0]), 0,
                                                       _p(out), 0))
        return out

    # ---- N1: cuckoo hashing for both parties (include/apsu_he.h: apsu_he_item_locations ... apsu_he_query_values)
    def _table_params(self):
        if not self.felts_per_item:
            raise ApsuHeError("context was created without PSUParams")
        return self.table_size, self.hash_func_count

    @staticmethod
    def _items16(items):
        return np.ascontiguousarray(items, dtype=np.uint8).reshape(-1, 16)

    def item_locations(self, items, count=None, locs=None):
        """Kuku's LocFunc for items [count][16] uint8 -> locs [count][hash_func_count] uint32 (apsu_he_item_locations).  items / locs
        may be device pointers (ints; `count` then says how many items): locs then stays on the device and None is returned."""
        T, H = self._table_params()
        on_dev = isinstance(items, int)
        if not on_dev:
            items = self._items16(items)
            count = items.shape[0]
        out = np.empty((count, H), dtype=np.uint32) if locs is None else None
        _check(load_library().apsu_he_item_locations(self.h, C.c_void_p(items if on_dev else items.ctypes.data), C.c_size_t(count), 1 if on_dev else 0,
                                                     C.c_void_p(out.ctypes.data if locs is None else int(locs)), 0 if locs is None else 1))
        return out

    def bucket_items(self, items):
        """the database side's grouping -> (offsets [table_size + 1] uint64, order uint32): order[offsets[l]:offsets[l + 1]] = the items
        with l among their locations, in input order, each once (apsu_he_items_bucket)"""
        T, H = self._table_params()
        items = self._items16(items)
        offsets = np.zeros(T + 1, dtype=np.uint64)
        order = np.zeros(max(items.shape[0] * H, 1), dtype=np.uint32)
        total = C.c_uint64()
        _check(load_library().apsu_he_items_bucket(self.h, C.c_void_p(items.ctypes.data), C.c_size_t(items.shape[0]), 0, _p(offsets),
                                                   C.c_void_p(order.ctypes.data), C.byref(total)))
        return offsets, order[:total.value].copy()

    def bucket_items_device(self, items, count=None, order=None, entries=None):
        """bucket_items with the grouping and the gather on the device (apsu_he_items_bucket_device) -> (offsets [table_size + 1] uint64,
        order [total] uint32, entries [total][16] uint8 = items[order], total).  items may be a device pointer (int; `count` then says how
        many items).  order / entries: True (the default, None, too) returns the array; False leaves it out (None in its place); a device
        pointer (int) with room for count * hash_func_count words / 16-byte entries is written to instead, and None is returned in its
        place.  Only offsets visit the host then."""
        T, H = self._table_params()
        on_dev = isinstance(items, int) and not isinstance(items, bool)
        if not on_dev:
            items = self._items16(items)
            count = items.shape[0]
        elif count is None:
            raise ValueError("bucket_items_device: a device pointer needs its count")
        is_ptr = lambda x: isinstance(x, int) and not isinstance(x, bool)
        want = lambda x: x is None or x is True
        room = max(count * H, 1)
        h_order = np.zeros(room, dtype=np.uint32) if want(order) else None
        h_entries = np.zeros((room, 16), dtype=np.uint8) if want(entries) else None
        offsets = np.zeros(T + 1, dtype=np.uint64)
        total = C.c_uint64()
        arg = lambda host, given: C.c_void_p(host.ctypes.data) if host is not None else C.c_void_p(int(given) if is_ptr(given) else None)
        _check(load_library().apsu_he_items_bucket_device(self.h, C.c_void_p(items if on_dev else items.ctypes.data), C.c_size_t(count), 1 if on_dev else 0,
                                                          _p(offsets), arg(h_order, order), 1 if is_ptr(order) else 0,
                                                          arg(h_entries, entries), 1 if is_ptr(entries) else 0, C.byref(total)))
        n = total.value
        return (offsets, None if h_order is None else h_order[:n].copy(), None if h_entries is None else h_entries[:n].copy(), n)

    def bucket_times(self):
        """-> (k_cuckoo_locations, the grouping, k_entries_gather) ms: device time of the last bucket_items_device call"""
        v = [C.c_double() for _ in range(3)]
        _check(load_library().apsu_he_debug_bucket_times(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def debug_bucket_locs(self, locs, table_size, tile_entries=0, order=None, offsets=None):
        """test hook: the device grouping alone on caller-given locations locs [count][H] -> (offsets [table_size + 1], order, total).
        order, offsets: arrays of count * H uint32 / table_size + 1 uint64 words to write into (the whole arrays are returned, so that a
        test sees the words past total, and what a refusal left)"""
        locs = np.ascontiguousarray(locs, dtype=np.uint32)
        if locs.ndim != 2 or not locs.shape[1]:
            raise ValueError("debug_bucket_locs: locs must be [count][H]")
        count, H = locs.shape
        if offsets is None:
            offsets = np.zeros(max(table_size, 0) + 1, dtype=np.uint64)
        if order is None:
            order = np.zeros(max(count * H, 1), dtype=np.uint32)
        assert order.dtype == np.uint32 and order.flags["C_CONTIGUOUS"] and order.size >= count * H
        total = C.c_uint64()
        _check(load_library().apsu_he_debug_bucket_locs(self.h, C.c_void_p(locs.ctypes.data), C.c_size_t(count), C.c_uint32(H), C.c_uint32(table_size),
                                                        C.c_uint32(tile_entries), _p(offsets), C.c_void_p(order.ctypes.data), C.byref(total)))
        return offsets, order, total.value

    def build_database_from_items(self, items, oprf=None):
        """The resident database of `items` [count][16]: bucket_items_device with gathered entries, then build_database.  oprf None: the
        entries stay on the device between the two calls.  Otherwise they are downloaded, oprf(entries [total][16], offsets) returns
        the post-OPRF entries [total][16], and the database is built from those.  -> the Bundles, as build_database returns them."""
        import torch
        T, H = self._table_params()
        items = self._items16(items)
        if oprf is None:
            buf = torch.empty(max(items.shape[0] * H, 1) * 16, dtype=torch.uint8, device="cuda:%d" % self.device)
            torch.cuda.synchronize(buf.device)
            offsets, _, _, total = self.bucket_items_device(items, order=False, entries=buf.data_ptr())
            return self.build_database(buf.data_ptr(), offsets)
        offsets, _, entries, total = self.bucket_items_device(items, order=False)
        hashed = self._items16(oprf(entries, offsets))
        if hashed.shape[0] != total:
            raise ValueError("build_database_from_items: oprf must return one entry per entry it was given")
        return self.build_database(hashed, offsets)

    def bucket_entries(self, offsets):
        """offsets of bucket_items -> per bundle index (lo, hi, start_bins): its entries are order[lo:hi] (contiguous, location by
        location) and start_bins [hi - lo] uint32 = (location % items_per_bundle) * felts_per_item of each"""
        T, _ = self._table_params()
        ipb = int(self.info.items_per_bundle)
        offsets = np.asarray(offsets, dtype=np.uint64)
        sizes = np.diff(offsets).astype(np.int64)
        out = []
        for b in range(self.bundle_idx_count):
            l0, l1 = b * ipb, (b + 1) * ipb
            start = np.repeat(((np.arange(l0, l1) % ipb) * self.felts_per_item).astype(np.uint32), sizes[l0:l1])
            out.append((int(offsets[l0]), int(offsets[l1]), start))
        return out

    def insert_items(self, bundles_by_index, items, oprf=None):
        """Items into a resident database: bucket_items -> oprf(per location, the list of its items [k][16]) -> one list of [k][16] per
        location, None: the items themselves -> algebraize_items -> apply_entries per bundle index.  bundles_by_index: {bundle index:
        its Bundles in cache order} (missing: none yet).  -> {bundle index: ApplyResult} for the bundle indices that got entries."""
        items = self._items16(items)
        offsets, order = self.bucket_items(items)
        per_loc = [items[order[int(offsets[l]):int(offsets[l + 1])]] for l in range(self.table_size)]
        if oprf is not None:
            per_loc = [self._items16(x) for x in oprf(per_loc)]
            if [len(x) for x in per_loc] != np.diff(offsets).astype(np.int64).tolist():
                raise ValueError("insert_items: oprf must return one item per item it was given, location by location")
        hashed = np.concatenate(per_loc) if per_loc else np.zeros((0, 16), dtype=np.uint8)
        felts = self.algebraize_items(hashed)
        out = {}
        for b, (lo, hi, start) in enumerate(self.bucket_entries(offsets)):
            if hi > lo:
                out[b] = self.apply_entries(list(bundles_by_index.get(b, [])), inserts=(felts[lo:hi], start), bundle_idx=b)
        return out

    # ---- N1: a whole database from its entries (include/apsu_he.h: apsu_he_db_build_from_entries)
    def _offsets(self, offsets):
        T, _ = self._table_params()
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if offsets.shape != (T + 1,):
            raise ValueError("offsets: table_size + 1 words, as bucket_items returns them")
        return offsets

    def entries_plan(self, offsets):
        """offsets of bucket_items -> BinBundles per bundle index [bundle_idx_count] uint32, as build_database will make them
        (apsu_he_db_entries_plan; the host half alone)"""
        offsets = self._offsets(offsets)
        per_index = np.zeros(self.bundle_idx_count, dtype=np.uint32)
        total = C.c_uint32()
        _check(load_library().apsu_he_db_entries_plan(self.h, _p(offsets), C.c_void_p(per_index.ctypes.data), C.byref(total)))
        assert int(per_index.sum()) == total.value
        return per_index

    def build_database(self, entries, offsets, count=None):
        """The resident database of the post-OPRF items entries [offsets[-1]][16] uint8, location by location in bucket_items' order ->
        its Bundles, bundle index by bundle index, in cache order within each (apsu_he_db_build_from_entries).  ReceiverDB::set_data
        on an empty database; no entry-level dedupe: two equal entries of one location are a double root of their bins.  entries
        may be a device pointer (int).  All or nothing."""
        offsets = self._offsets(offsets)
        per_index = self.entries_plan(offsets)
        total = int(per_index.sum())
        on_dev = isinstance(entries, int)
        if not on_dev:
            entries = self._items16(entries)
            if entries.shape[0] != int(offsets[-1]):
                raise ValueError("build_database: %d entries, offsets name %d" % (entries.shape[0], int(offsets[-1])))
        hs = (C.c_void_p * max(total, 1))()
        n_out = C.c_uint32()
        _check(load_library().apsu_he_db_build_from_entries(self.h, C.c_void_p(entries if on_dev else entries.ctypes.data), 1 if on_dev else 0, _p(offsets),
                                                            hs, C.c_uint32(total if count is None else int(count)), C.byref(n_out)))
        assert n_out.value == total
        ids = [(b, k) for b in range(self.bundle_idx_count) for k in range(int(per_index[b]))]
        return [self._wrap_new(hs[i], b, k) for i, (b, k) in enumerate(ids)]

    def build_times(self):
        """-> (the entries' copies, k_entries_scatter, the builds) ms: device time of the last build_database call, summed over its
        bundle indices and BinBundles"""
        v = [C.c_double() for _ in range(3)]
        _check(load_library().apsu_he_debug_build_from_entries_times(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def set_scatter_blocks(self, blocks):
        """measurements: workgroups per location of k_entries_scatter in the build_database calls that follow; 0 = the engine's choice"""
        _check(load_library().apsu_he_debug_set_scatter_blocks(self.h, C.c_uint32(blocks)))

    def cuckoo_table(self, items, max_rounds=500):
        """the querier's table by the engine's deterministic rule -> (table_idx [table_size] uint32: item or 0xFFFFFFFF, item_loc
        [count] uint32: location, 0xFFFFFFFF for a repeated item, rounds); apsu_he_cuckoo_table.  An item without a slot after
        max_rounds: ApsuHeError naming the lowest one and the fill rate."""
        T, _ = self._table_params()
        items = self._items16(items)
        table_idx = np.zeros(T, dtype=np.uint32)
        item_loc = np.zeros(max(items.shape[0], 1), dtype=np.uint32)
        rounds = C.c_uint64()
        _check(load_library().apsu_he_cuckoo_table(self.h, C.c_void_p(items.ctypes.data), C.c_size_t(items.shape[0]), 0, C.c_uint64(max_rounds),
                                                   C.c_void_p(table_idx.ctypes.data), C.c_void_p(item_loc.ctypes.data), C.byref(rounds)))
        return table_idx, item_loc[:items.shape[0]], rounds.value

    def debug_item_locations(self, items, hash_func_count, table_size):
        """test hook: k_cuckoo_locations with a caller-given function count and table size -> locs [count][hash_func_count]"""
        items = self._items16(items)
        out = np.empty((items.shape[0], hash_func_count), dtype=np.uint32)
        _check(load_library().apsu_he_debug_item_locations(self.h, C.c_void_p(items.ctypes.data), C.c_size_t(items.shape[0]), C.c_uint32(hash_func_count),
                                                           C.c_uint32(table_size), C.c_void_p(out.ctypes.data)))
        return out

    def debug_cuckoo_insert(self, items, locs, table_size, max_rounds=500, form=0):
        """test hook: the table rule on caller-given locations locs [count][H]; form 0 the engine's choice, 1 LDS, 2 device memory"""
        items = self._items16(items)
        locs = np.ascontiguousarray(locs, dtype=np.uint32)
        if locs.ndim != 2 or locs.shape[0] != items.shape[0] or not locs.shape[1]:
            raise ValueError("debug_cuckoo_insert: locs must be [count][H]")
        table_idx = np.zeros(max(table_size, 1), dtype=np.uint32)
        item_loc = np.zeros(max(items.shape[0], 1), dtype=np.uint32)
        rounds = C.c_uint64()
        _check(load_library().apsu_he_debug_cuckoo_insert(self.h, C.c_void_p(items.ctypes.data), C.c_void_p(locs.ctypes.data), C.c_size_t(items.shape[0]),
                                                          C.c_uint32(locs.shape[1]), C.c_uint32(table_size), C.c_uint64(max_rounds), int(form),
                                                          C.c_void_p(table_idx.ctypes.data), C.c_void_p(item_loc.ctypes.data), C.byref(rounds)))
        return table_idx[:table_size], item_loc[:items.shape[0]], rounds.value

    def query_values(self, table_items, values=None):
        """table_items [table_size][16] uint8, the table after the caller's OPRF (or a device pointer) -> values [bundle_idx_count][n]
        as query_create reads them; values: a device pointer to write them to instead (None is returned).  apsu_he_query_values"""
        T, _ = self._table_params()
        on_dev = isinstance(table_items, int)
        if not on_dev:
            table_items = self._items16(table_items)
            if table_items.shape[0] != T:
                raise ValueError("query_values: table_items must hold table_size items")
        out = np.empty((self.bundle_idx_count, self.n), dtype=np.uint64) if values is None else None
        _check(load_library().apsu_he_query_values(self.h, C.c_void_p(table_items if on_dev else table_items.ctypes.data), 1 if on_dev else 0,
                                                   _p(out) if values is None else C.c_void_p(int(values)), 0 if values is None else 1))
        return out

    def save_db_file(self, path, bundles):
        """the whole DB (these BinBundles, in this order) into one mmap-able file (ReceiverDB::save counterpart)"""
        hs = (C.c_void_p * len(bundles))(*[b.h for b in bundles])
        _check(load_library().apsu_he_db_file_save(self.h, os.fsencode(path), hs, len(bundles)))

    def load_db_file(self, path, only=None):
        """-> [Bundle] of the file's BinBundles (all, or the table positions in `only`), loaded onto this context's device"""
        with DbFile(path) as f:
            return [f.load(self, i) for i in (range(len(f)) if only is None else only)]

    def save_bundle(self, bundle):
        """-> bytes: engine-native image of the BinBundle cache (ReceiverDB::save counterpart)"""
        size = C.c_uint64()
        _check(load_library().apsu_he_bundle_image_size(self.h, bundle.h, C.byref(size)))
        buf = np.empty(size.value, dtype=np.uint8)
        wr = C.c_uint64()
        _check(load_library().apsu_he_bundle_save(self.h, bundle.h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), size, C.byref(wr)))
        return buf[: wr.value]

    def load_bundle(self, image):
        """image: bytes / uint8 array / np.memmap produced by save_bundle (ReceiverDB::Load counterpart)"""
        arr = np.ascontiguousarray(np.frombuffer(image, dtype=np.uint8) if not isinstance(image, np.ndarray) else image)
        h = C.c_void_p()
        _check(load_library().apsu_he_bundle_load(self.h, arr.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_uint64(arr.size), C.byref(h)))
        deg = C.c_uint32()
        _check(load_library().apsu_he_bundle_degree(h, C.byref(deg)))
        return Bundle(self, h, -1, -1, deg.value)

    def set_two_stream(self, mode):
        """-1 default policy, 0 off, 1 on: ComputePowers' high-power chain on a second stream"""
        _check(load_library().apsu_he_set_two_stream(self.h, int(mode)))

    def set_async_results(self, on):
        """eval_bundles with device-resident masks and output returns once its work is queued; see sync() / stream"""
        _check(load_library().apsu_he_set_async_results(self.h, int(bool(on))))

    def set_query_overlap(self, mode):
        """apsu_he_set_query_overlap: the device-resident inputs of compute_powers are complete when it is called (not produced by
        work queued on the context's stream), so consecutive queued queries may overlap.  False / 0 off, True / 1 on, 2 on without
        the pipelined walk, 3 on with the pipelined walk forced (tests)"""
        _check(load_library().apsu_he_set_query_overlap(self.h, int(mode)))

    def set_tier1_on_device(self, on):
        """tier-1 calls take device pointers (ints) and only queue their work; see sync() / stream"""
        _check(load_library().apsu_he_set_tier1_on_device(self.h, int(bool(on))))

    def sync(self):
        """wait for everything this context has queued"""
        _check(load_library().apsu_he_sync(self.h))

    @property
    def stream(self):
        """the context's main HIP stream as an integer handle (e.g. for torch.cuda.ExternalStream)"""
        p = C.c_void_p()
        _check(load_library().apsu_he_stream(self.h, C.byref(p)))
        return int(p.value or 0)

    def mask_generate(self, seed, count, masks_dev, want_values=True, want_blocks=True):
        """N4: `count` random masks (receiver_osn.cpp:217-284).  masks_dev: device pointer to count*n words receiving the
        encoded plaintexts.  -> (values [count][n] or None, blocks [count][items_per_bundle][2] (low, high) or None)"""
        vals = np.empty((count, self.n), dtype=np.uint64) if want_values else None
        blks = np.empty((count, self.info.items_per_bundle, 2), dtype=np.uint64) if want_blocks else None
        _check(load_library().apsu_he_mask_generate(self.h, C.c_uint64(seed), C.c_uint32(count), C.c_void_p(int(masks_dev)),
                                                    _p(vals) if want_values else None, _p(blks) if want_blocks else None))
        return vals, blks

    def mask_generate_blake2xb(self, seed, count, masks_dev, first_value=0, want_values=True, want_blocks=True):
        """N4 with the reference's generator: SEAL's Blake2xb PRNG under the eight 64-bit words `seed`
        (receiver_osn.cpp:221-224, 248-251), starting at its first_value-th 32-bit output.  Same outputs as mask_generate."""
        sd = np.ascontiguousarray(seed, dtype=np.uint64)
        if sd.size != 8:
            raise ValueError("seed must be eight 64-bit words")
        vals = np.empty((count, self.n), dtype=np.uint64) if want_values else None
        blks = np.empty((count, self.info.items_per_bundle, 2), dtype=np.uint64) if want_blocks else None
        _check(load_library().apsu_he_mask_generate_blake2xb(self.h, _p(sd), C.c_uint64(first_value), C.c_uint32(count),
                                                             C.c_void_p(int(masks_dev)), _p(vals) if want_values else None,
                                                             _p(blks) if want_blocks else None))
        return vals, blks

    def decrypt_decode(self, sk_ntt, cts, count=None, on_device=False, want_blocks=True, want_budget=False):
        """N4: the querier's decrypt + decode + packing of `count` results (result_package.cpp:175-213).
        sk_ntt: secret key mod q_0 in NTT form [n]; cts: [count][2][1][n] array, or a device pointer with on_device.
        want_budget: a third return value, SEAL's invariant noise budget (bits, int32) of every result."""
        if not on_device:
            cts = np.ascontiguousarray(cts, dtype=np.uint64)
            count = cts.size // (2 * self.n)
            ptr = _p(cts)
        else:
            ptr = C.c_void_p(int(cts))
        vals = np.empty((count, self.n), dtype=np.uint64)
        blks = np.empty((count, self.info.items_per_bundle, 2), dtype=np.uint64) if want_blocks else None
        sk = np.ascontiguousarray(sk_ntt, dtype=np.uint64)
        if want_budget:
            bits = np.zeros(count, dtype=np.int32)
            _check(load_library().apsu_he_decrypt_decode_budget(self.h, _p(sk), ptr, 1 if on_device else 0, C.c_uint32(count), _p(vals),
                                                                _p(blks) if want_blocks else None, C.c_void_p(bits.ctypes.data)))
            return vals, blks, bits
        _check(load_library().apsu_he_decrypt_decode(self.h, _p(sk), ptr, 1 if on_device else 0, C.c_uint32(count), _p(vals),
                                                     _p(blks) if want_blocks else None))
        return vals, blks

    # ---- N5: the querier's side (Sender::reset_keys, Sender::create_query; sender/apsu/sender_osn.cpp:215-229,426-484)
    @staticmethod
    def _seed_words(seed):
        """64 bytes or eight 64-bit words; None: fresh from the operating system (the seed is key material)"""
        if seed is None:
            seed = os.urandom(64)
        if isinstance(seed, (bytes, bytearray)):
            if len(seed) != 64:
                raise ValueError("seed must be 64 bytes")
            return np.frombuffer(bytes(seed), dtype="<u8").astype(np.uint64)
        sd = np.ascontiguousarray(seed, dtype=np.uint64)
        if sd.size != 8:
            raise ValueError("seed must be eight 64-bit words")
        return sd

    def keygen(self, seed=None):
        """-> sk_ntt [K][n]: a uniform ternary secret modulo every key prime, NTT form (sk_ntt[0] is what decrypt_decode takes)"""
        sd = self._seed_words(seed)
        sk = np.empty((self.K, self.n), dtype=np.uint64)
        _check(load_library().apsu_he_keygen(self.h, _p(sd), _p(sk)))
        return sk

    def relin_keygen(self, sk_ntt, seed=None, want_host=True, want_resident=True):
        """-> (ksk [K-1][2][K][n] or None, public seeds [K-1][8], RelinKeys resident on the device or None)"""
        sd = self._seed_words(seed)
        sk = np.ascontiguousarray(sk_ntt, dtype=np.uint64)
        if sk.size != self.K * self.n:
            raise ValueError("sk_ntt must hold K * n words")
        nk = max(self.K - 1, 0)
        ksk = np.empty((nk, 2, self.K, self.n), dtype=np.uint64) if want_host else None
        seeds = np.empty((nk, 8), dtype=np.uint64)
        h = C.c_void_p()
        _check(load_library().apsu_he_relin_keygen(self.h, _p(sk), _p(sd), _p(ksk) if want_host else None, _p(seeds),
                                                   C.byref(h) if want_resident else None))
        return ksk, seeds, (RelinKeys(self, h) if want_resident else None)

    def query_create(self, sk_ntt, bundle_indices, values, cts_dev, seed=None, values_on_device=False):
        """Encrypted source powers of a query.  values: [len(bundle_indices)][n] slot values (< t), or a device pointer with
        values_on_device; cts_dev: device pointer to len(bundle_indices) * source_power_count * 2 * (first_chain_idx + 1) * n words,
        ciphertext b * source_power_count + s = source power s (ascending) of bundle_indices[b], as compute_powers(on_device=True)
        reads them.  -> public seeds [count][8] of the ciphertexts' c1."""
        sd = self._seed_words(seed)
        sk = np.ascontiguousarray(sk_ntt, dtype=np.uint64)
        if sk.size < (self.first_chain_idx + 1) * self.n:
            raise ValueError("sk_ntt must hold the limbs of the first data level")
        idx = np.array(bundle_indices, dtype=np.uint32)
        if values_on_device:
            vp = C.c_void_p(int(values))
        else:
            values = np.ascontiguousarray(values, dtype=np.uint64)
            if values.size != len(idx) * self.n:
                raise ValueError("values must hold n slot values per bundle index")
            vp = _p(values)
        seeds = np.empty((len(idx) * self.source_power_count, 8), dtype=np.uint64)
        _check(load_library().apsu_he_query_create(self.h, _p(sk), _p(sd), C.c_void_p(idx.ctypes.data), len(idx), vp,
                                                   1 if values_on_device else 0, C.c_void_p(int(cts_dev)), _p(seeds)))
        return seeds

    def bundle_coeff(self, bundle, degree):
        """test hook -> (array, kind): kind 0 raw mod t, 1 NTT form [L][n], 2 pre-lifted NTT at the high level"""
        buf = np.empty((self.first_chain_idx + 1) * self.n, dtype=np.uint64)
        words, kind = C.c_size_t(), C.c_int()
        _check(load_library().apsu_he_bundle_download(self.h, bundle.h, degree, _p(buf), C.c_size_t(buf.size), C.byref(words),
                                                      C.byref(kind)))
        w = words.value
        return (buf[:w].copy() if kind.value == 0 else buf[:w].reshape(-1, self.n).copy()), kind.value

    def random_bundle(self, bundle_idx, cache_idx, degree, seed):
        h = C.c_void_p()
        _check(load_library().apsu_he_db_random_bundle(self.h, bundle_idx, cache_idx, degree, C.c_uint64(seed), C.byref(h)))
        return Bundle(self, h, bundle_idx, cache_idx, degree)

    def compute_powers(self, bundle_indices, sources, rk, on_device=False):
        """Receiver::ComputePowers.  sources[b][s]: ct (numpy [2][L][n]) or device pointer (int) of the
        s-th source power (ascending) for bundle index bundle_indices[b]."""
        idx = np.array(bundle_indices, dtype=np.uint32)
        flat = [s for per_b in sources for s in per_b]
        h = C.c_void_p()
        _check(load_library().apsu_he_compute_powers(self.h, C.c_void_p(idx.ctypes.data), len(idx), _ptr_array(flat),
                                                     1 if on_device else 0, rk.h if rk is not None else None, C.byref(h)))
        return Powers(self, h, bundle_indices)

    def eval_bundles(self, bundles, powers, rk, masks, out=None, masks_on_device=False, out_on_device=False):
        """ProcessBinBundleCache for every bundle: returns [count][2][1][n] (host) unless out is a device pointer.
        Without key switching a row has result_polys polynomials, result i being its first result_size(bundle i) ones."""
        count = len(bundles)
        hs = (C.c_void_p * count)(*[b.h for b in bundles])
        if not out_on_device:
            out = np.empty((count, self.result_polys, 1, self.n), dtype=np.uint64)
            outp = _p(out)
        else:
            outp = C.c_void_p(int(out))
        _check(load_library().apsu_he_eval_bundles(self.h, hs, count, powers.h, rk.h if rk is not None else None,
                                                   _ptr_array(list(masks)), 1 if masks_on_device else 0, outp,
                                                   1 if out_on_device else 0))
        return out


class DbFile:
    """a database file opened with mmap: the table, and BinBundles loaded one by one (apsu_he_db_file_*)"""

    def __init__(self, path):
        self.h = C.c_void_p()
        _check(load_library().apsu_he_db_file_open(os.fsencode(path), C.byref(self.h)))
        cnt, size = C.c_int(), C.c_uint64()
        _check(load_library().apsu_he_db_file_count(self.h, C.byref(cnt), C.byref(size)))
        self.count, self.file_bytes = cnt.value, size.value

    def __len__(self):
        return self.count

    def entry(self, i):
        """-> (bundle_idx, cache_idx, degree, image_bytes)"""
        b, c, d, sz = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        _check(load_library().apsu_he_db_file_entry(self.h, int(i), C.byref(b), C.byref(c), C.byref(d), C.byref(sz)))
        return b.value, c.value, d.value, sz.value

    def load(self, ctx, i):
        h = C.c_void_p()
        _check(load_library().apsu_he_db_file_load(ctx.h, self.h, int(i), C.byref(h)))
        b, c, d, _ = self.entry(i)
        return Bundle(ctx, h, b, c, d)

    def close(self):
        if getattr(self, "h", None):
            load_library().apsu_he_db_file_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def partition_bundles(units, bundle_idx_count, n_devices, compute_powers_cost=0):
    """apsu_he_partition_bundles(_ex): units [(bundle_idx, cache_idx, degree)] -> device slot per unit (no GPU needed)"""
    cnt = len(units)
    b = np.array([u[0] for u in units] or [0], dtype=np.uint32)
    c = np.array([u[1] for u in units] or [0], dtype=np.uint32)
    d = np.array([u[2] for u in units] or [0], dtype=np.uint32)
    out = np.zeros(max(cnt, 1), dtype=np.int32)
    _check(load_library().apsu_he_partition_bundles_ex(C.c_uint32(bundle_idx_count), int(n_devices), C.c_void_p(b.ctypes.data),
                                                       C.c_void_p(c.ctypes.data), C.c_void_p(d.ctypes.data), cnt,
                                                       C.c_uint64(int(compute_powers_cost)), C.c_void_p(out.ctypes.data)))
    return [int(x) for x in out[:cnt]]


class MultiContext:
    """Several GPUs of one node behind one handle (include/apsu_he.h: apsu_he_multi_*, apsu_he_eval_all): the
    in-process counterpart of Receiver::RunQuery's fan-out (receiver/apsu/receiver_osn.cpp:320-364)."""

    def __init__(self, psu_params_json, devices):
        L = load_library()
        if os.path.exists(psu_params_json):
            with open(psu_params_json) as f:
                psu_params_json = f.read()
        dv = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        _check(L.apsu_he_multi_create(psu_params_json.encode(), dv, len(devices), C.byref(h)))
        self.h = h
        self.devices = list(devices)
        self.n_bundles = 0
        js = json.loads(psu_params_json)
        self.felts_per_item = int(js["item_params"]["felts_per_item"])
        self.n = int(js["seal_params"]["poly_modulus_degree"])
        rp = C.c_uint32()
        _check(L.apsu_he_multi_result_polys(self.h, C.byref(rp)))
        self.result_polys = rp.value

    def close(self):
        if getattr(self, "h", None):
            load_library().apsu_he_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload_relin_keys(self, rk):
        _check(load_library().apsu_he_multi_relin_upload(self.h, _p(np.ascontiguousarray(rk))))

    def upload_bundle(self, slot, bundle_idx, cache_idx, coeffs, is_ntt):
        flags = (C.c_uint8 * len(coeffs))(*[1 if f else 0 for f in is_ntt])
        keep = [np.ascontiguousarray(c, dtype=np.uint64) for c in coeffs]
        bid = C.c_int()
        _check(load_library().apsu_he_multi_db_upload_bundle(self.h, int(slot), bundle_idx, cache_idx, len(keep), _ptr_array(keep),
                                                             flags, C.byref(bid)))
        self.n_bundles = max(self.n_bundles, bid.value + 1)
        return bid.value

    def random_bundle(self, slot, bundle_idx, cache_idx, degree, seed):
        bid = C.c_int()
        _check(load_library().apsu_he_multi_db_random_bundle(self.h, int(slot), bundle_idx, cache_idx, degree, C.c_uint64(seed),
                                                             C.byref(bid)))
        self.n_bundles = max(self.n_bundles, bid.value + 1)
        return bid.value

    def update_bundle(self, bundle_id, inserts=None, removes=None):
        """HeContext.update_bundle on BinBundle `bundle_id`, on its device; it keeps its id (its row of eval_all)"""
        args, keep, nb = _update_lists(inserts, removes)
        _check(load_library().apsu_he_multi_db_update_bundle(self.h, int(bundle_id), *args, nb))

    def clear_bundles(self):
        _check(load_library().apsu_he_multi_db_clear(self.h))
        self.n_bundles = 0

    # ---- the resident database maintained on the handle (include/apsu_he.h: apsu_he_multi_db_*).  Ids stay dense: a call that drops
    # BinBundles returns new_id (old id -> id from now on, -1 for a dropped one), and n_bundles follows.
    def bundle_count(self):
        k = C.c_int()
        _check(load_library().apsu_he_multi_db_bundle_count(self.h, C.byref(k)))
        self.n_bundles = k.value
        return k.value

    def bundle_info(self, bundle_id):
        """-> BundleInfo(slot, bundle_idx, cache_idx, degree)"""
        slot, b, c, d = C.c_int(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(load_library().apsu_he_multi_db_bundle_info(self.h, int(bundle_id), C.byref(slot), C.byref(b), C.byref(c), C.byref(d)))
        return BundleInfo(slot.value, b.value, c.value, d.value)

    def index_bundles(self, bundle_idx):
        """-> the ids of one bundle index in cache order (ascending cache_idx)"""
        cap = max(self.bundle_count(), 1)
        ids = (C.c_int * cap)()
        k = C.c_int()
        _check(load_library().apsu_he_multi_db_index_bundles(self.h, C.c_uint32(bundle_idx), ids, cap, C.byref(k)))
        return [int(v) for v in ids[:k.value]]

    def bin_counts(self, bundle_id):
        """HeContext.bin_counts of BinBundle `bundle_id`, on its device"""
        counts = np.empty(self.n, dtype=np.uint32)
        _check(load_library().apsu_he_multi_db_bin_counts(self.h, int(bundle_id), C.c_void_p(counts.ctypes.data)))
        return counts

    def bins(self, bundle_id):
        """HeContext.bins of BinBundle `bundle_id`, on its device (apsu_he_multi_db_bundle_bins)"""
        counts = self.bin_counts(bundle_id)
        stride = _bins_stride(counts)
        roots = np.zeros((len(counts), stride), dtype=np.uint64)
        _check(load_library().apsu_he_multi_db_bundle_bins(self.h, int(bundle_id), _p(roots), C.c_void_p(counts.ctypes.data), C.c_uint32(stride)))
        return _bins_list(roots, counts)

    def self_test(self, seed=None):
        """HeContext.self_test of every registered BinBundle, each device testing its own, devices side by side
        (apsu_he_multi_db_self_test) -> SelfTestReport; BinBundles are named by id"""
        sd = HeContext._seed_words(seed)
        rep = _SelfTestReport()
        _check(load_library().apsu_he_multi_db_self_test(self.h, _p(sd), C.byref(rep)))
        return _self_test_report(rep)

    def build_bundle(self, bundle_idx, cache_idx, bins, slot=-1):
        """HeContext.build_bundle on `slot`, or (slot -1) on the slot the placement rule chooses -> the new id (registered last)"""
        nb = len(bins)
        stride = max([len(b) for b in bins] + [1])
        roots = np.zeros((max(nb, 1), stride), dtype=np.uint64)
        counts = np.zeros(max(nb, 1), dtype=np.uint32)
        for i, b in enumerate(bins):
            counts[i] = len(b)
            roots[i, :len(b)] = b
        bid = C.c_int()
        _check(load_library().apsu_he_multi_db_build_bundle(self.h, int(slot), C.c_uint32(bundle_idx), C.c_uint32(cache_idx), _p(roots),
                                                            C.c_void_p(counts.ctypes.data), nb, stride, C.byref(bid)))
        self.n_bundles = bid.value + 1
        return bid.value

    def _renumbered(self, call, extra=0):
        """runs call(new_id pointer) with room for the ids before the call (+ extra) -> new_id as a list; n_bundles follows"""
        before = self.bundle_count()
        new_id = np.full(before + extra, -2, dtype=np.int32)
        keep = call(C.c_void_p(new_id.ctypes.data) if len(new_id) else None)
        self.bundle_count()
        return [int(v) for v in new_id], keep

    def remove_bundle(self, bundle_id):
        """drops one BinBundle -> new_id"""
        return self._renumbered(lambda p: _check(load_library().apsu_he_multi_db_remove_bundle(self.h, int(bundle_id), p)))[0]

    def move_bundle(self, bundle_id, slot):
        """the BinBundle's arrays go to `slot`, device to device; it keeps its id"""
        _check(load_library().apsu_he_multi_db_move_bundle(self.h, int(bundle_id), int(slot)))

    def lookup(self, bundle_idx, entries):
        """HeContext.lookup against the BinBundles of index_bundles(bundle_idx), rows in that order -> (present, room)"""
        felts, start = _entries(entries, self.felts_per_item)
        rows = len(self.index_bundles(bundle_idx))
        present = np.zeros((rows, len(start)), dtype=np.uint8)
        room = np.zeros((rows, len(start)), dtype=np.uint32)
        _check(load_library().apsu_he_multi_db_lookup(self.h, C.c_uint32(bundle_idx), _p(felts), C.c_void_p(start.ctypes.data), C.c_size_t(len(start)),
                                                      C.c_void_p(present.ctypes.data), C.c_void_p(room.ctypes.data)))
        return present.astype(bool), room

    def apply_entries(self, bundle_idx, inserts=None, removes=None):
        """HeContext.apply_entries on index_bundles(bundle_idx) -> MultiApplyResult: new_id [ids before the call + n_appended], and per
        entry status (ENTRY_*) and target = an OLD id (the k-th appended BinBundle: ids before the call + k)"""
        fi, si = _entries(inserts, self.felts_per_item)
        fr, sr = _entries(removes, self.felts_per_item)
        n_app = C.c_uint32()
        out = [np.zeros(len(si), dtype=np.uint32), np.zeros(len(si), dtype=np.uint32), np.zeros(len(sr), dtype=np.uint32), np.zeros(len(sr), dtype=np.uint32)]
        u32 = lambda a: C.c_void_p(a.ctypes.data)
        L = load_library()
        new_id, _ = self._renumbered(lambda p: _check(L.apsu_he_multi_db_apply_entries(
            self.h, C.c_uint32(bundle_idx), _p(fi), u32(si), C.c_size_t(len(si)), _p(fr), u32(sr), C.c_size_t(len(sr)), p, C.byref(n_app),
            *[u32(a) for a in out])), extra=len(si))
        return MultiApplyResult(new_id[:len(new_id) - len(si) + n_app.value], n_app.value, *out)

    def build_database(self, entries, offsets):
        """HeContext.build_database on the handle (host entries): BinBundle (bundle index, k) on the slot the placement rule gives
        it, in that order -> the new ids, appended densely.  Refused where the handle already holds a BinBundle of a bundle index
        that receives entries.  All or nothing."""
        entries = np.ascontiguousarray(entries, dtype=np.uint8).reshape(-1, 16)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if offsets.ndim != 1 or not len(offsets) or entries.shape[0] != int(offsets[-1]):
            raise ValueError("build_database: entries and offsets do not match")
        first, built = C.c_int(), C.c_uint32()
        _check(load_library().apsu_he_multi_db_build_from_entries(self.h, C.c_void_p(entries.ctypes.data), _p(offsets), C.byref(first), C.byref(built)))
        self.bundle_count()
        return list(range(first.value, first.value + built.value))

    def merge_bundles(self, bundle_ids):
        """HeContext.merge_bundles on BinBundles of one bundle index, wherever they lie -> new_id (the merged BinBundle takes the place
        of the first member in cache order)"""
        ids = (C.c_int * max(len(bundle_ids), 1))(*[int(i) for i in bundle_ids])
        return self._renumbered(lambda p: _check(load_library().apsu_he_multi_db_merge_bundles(self.h, ids, len(bundle_ids), p)))[0]

    def compact(self, bundle_idx):
        """HeContext.compact on index_bundles(bundle_idx) -> (new_id, merged BinBundles made)"""
        made = C.c_uint32()
        new_id, _ = self._renumbered(lambda p: _check(load_library().apsu_he_multi_db_compact(self.h, C.c_uint32(bundle_idx), p, C.byref(made))))
        return new_id, made.value

    def load_db_file(self, path):
        """every BinBundle of the file onto the handle's devices (partition rule, each device reads its own shard) -> count"""
        with DbFile(path) as f:
            k = C.c_int()
            _check(load_library().apsu_he_multi_db_load_file(self.h, f.h, C.byref(k)))
        self.n_bundles += k.value
        return k.value

    def save_db_file(self, path):
        _check(load_library().apsu_he_multi_db_save_file(self.h, os.fsencode(path)))

    IO_SRC_PINNED, IO_MASKS_PINNED, IO_OUT_PINNED, IO_SRC_ON_DEVICE, IO_MASKS_ON_DEVICE, IO_GATHER_RCCL = 1, 2, 4, 8, 16, 32

    def eval_all(self, sources, masks, n, out_device_slot=-1, out_ptr=None, flags=0, in_device_slot=0, out=None):
        """sources: flat list [bundle_idx][source] of cts (numpy arrays, or device pointers as ints with IO_SRC_ON_DEVICE);
        masks: per bundle id (likewise).  -> [n_bundles][2][1][n] (host; `out` = a caller-provided, e.g. page-locked, array)
        or writes to the device pointer out_ptr on devices[out_device_slot]"""
        if out_device_slot < 0:
            if out is None:
                out = np.zeros((self.n_bundles, self.result_polys, 1, n), dtype=np.uint64)
            outp = _p(out)
        else:
            out = None
            outp = C.c_void_p(int(out_ptr))
        _check(load_library().apsu_he_eval_all_ex(self.h, _ptr_array(list(sources)), _ptr_array(list(masks)), outp, int(out_device_slot),
                                                  C.c_uint(int(flags)), int(in_device_slot)))
        return out

    def last_gather(self):
        L = load_library()
        L.apsu_he_multi_last_gather.restype = C.c_char_p
        return L.apsu_he_multi_last_gather(self.h).decode()

    def phase_enable(self, on=True):
        _check(load_library().apsu_he_multi_phase_enable(self.h, 1 if on else 0))

    def phase_read(self, reset=True):
        L = load_library()
        L.apsu_he_phase_name.restype = C.c_char_p
        cnt = (C.c_uint64 * 3)(); avg = (C.c_double * 3)(); mn = (C.c_double * 3)(); mx = (C.c_double * 3)()
        _check(L.apsu_he_multi_phase_read(self.h, cnt, avg, mn, mx, 1 if reset else 0))
        return {L.apsu_he_phase_name(i).decode(): (int(cnt[i]), avg[i], mn[i], mx[i]) for i in range(3)}


def host_alloc(shape, dtype=np.uint64):
    """page-locked host array (apsu_he_host_alloc); release with host_free(array)"""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = C.c_void_p()
    _check(load_library().apsu_he_host_alloc(C.c_size_t(max(1, nbytes)), C.byref(p)))
    buf = (C.c_uint8 * max(1, nbytes)).from_address(p.value)
    a = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    _PINNED[a.ctypes.data] = p.value
    return a


def host_free(a):
    p = _PINNED.pop(a.ctypes.data, None)
    if p is not None:
        _check(load_library().apsu_he_host_free(C.c_void_p(p)))


_PINNED = {}
