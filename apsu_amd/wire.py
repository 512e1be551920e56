"""ctypes binding of the N3 framing functions (include/apsu_he.h: apsu_he_wire_*): the reference's FlatBuffers messages
around the query-evaluation path (common/apsu/network/*.fbs, receiver_operation.cpp, result_package.cpp).  Host only."""
import ctypes as C

from .engine import _check, load_library

u8p = C.POINTER(C.c_uint8)


def _take(out, size):
    data = C.string_at(out, size.value)
    load_library().apsu_he_wire_buffer_free(out)
    return data


def _buf(b):
    return (C.c_uint8 * len(b)).from_buffer_copy(b) if len(b) else (C.c_uint8 * 1)()


def build_header(version, rop_type):
    out, size = u8p(), C.c_size_t()
    _check(load_library().apsu_he_wire_build_header(version, rop_type, C.byref(out), C.byref(size)))
    return _take(out, size)


def parse_header(buf):
    v, t = C.c_uint32(), C.c_uint32()
    _check(load_library().apsu_he_wire_parse_header(_buf(buf), C.c_size_t(len(buf)), C.byref(v), C.byref(t)))
    return v.value, t.value


def build_query_request(compression_type, relin_keys, parts):
    """parts: [(exponent, [ct bytes, ...]), ...]; relin_keys: bytes or None"""
    flat = [ct for _, cts in parts for ct in cts]
    keep = [_buf(ct) for ct in flat]
    ptrs = (C.c_void_p * max(1, len(flat)))(*[C.addressof(k) for k in keep])
    sizes = (C.c_size_t * max(1, len(flat)))(*[len(ct) for ct in flat])
    exps = (C.c_uint32 * max(1, len(parts)))(*[e for e, _ in parts])
    cnts = (C.c_uint32 * max(1, len(parts)))(*[len(c) for _, c in parts])
    rk = _buf(relin_keys) if relin_keys is not None else None
    out, size = u8p(), C.c_size_t()
    _check(load_library().apsu_he_wire_build_query_request(C.c_uint8(compression_type), rk, C.c_size_t(len(relin_keys) if relin_keys is not None else 0),
                                                           len(parts), exps, cnts, ptrs, sizes, C.byref(out), C.byref(size)))
    return _take(out, size)


def parse_query_request(buf):
    """-> (compression_type, relin_keys bytes or None, [(exponent, [ct bytes])])"""
    L = load_library()
    keep = _buf(buf)
    h = C.c_void_p()
    _check(L.apsu_he_wire_parse_query_request(keep, C.c_size_t(len(buf)), C.byref(h)))
    try:
        ct, has, rk, rkn, nparts = C.c_uint8(), C.c_int(), u8p(), C.c_size_t(), C.c_uint32()
        _check(L.apsu_he_wire_query_info(h, C.byref(ct), C.byref(has), C.byref(rk), C.byref(rkn), C.byref(nparts)))
        relin = C.string_at(rk, rkn.value) if has.value else None
        parts = []
        for i in range(nparts.value):
            e, n = C.c_uint32(), C.c_uint32()
            _check(L.apsu_he_wire_query_part(h, i, C.byref(e), C.byref(n)))
            cts = []
            for j in range(n.value):
                p, sz = u8p(), C.c_size_t()
                _check(L.apsu_he_wire_query_ct(h, i, j, C.byref(p), C.byref(sz)))
                cts.append(C.string_at(p, sz.value))
            parts.append((e.value, cts))
        return ct.value, relin, parts
    finally:
        L.apsu_he_wire_query_free(h)


def build_query_response(package_count, alpha_max_cache_count):
    out, size = u8p(), C.c_size_t()
    _check(load_library().apsu_he_wire_build_query_response(package_count, alpha_max_cache_count, C.byref(out), C.byref(size)))
    return _take(out, size)


def parse_query_response(buf):
    a, b = C.c_uint32(), C.c_uint32()
    _check(load_library().apsu_he_wire_parse_query_response(_buf(buf), C.c_size_t(len(buf)), C.byref(a), C.byref(b)))
    return a.value, b.value


def build_result_package(bundle_idx, cache_idx, psu_result, label_byte_count=0, nonce_byte_count=0, labels=()):
    keep = [_buf(x) for x in labels]
    ptrs = (C.c_void_p * max(1, len(labels)))(*[C.addressof(k) for k in keep])
    sizes = (C.c_size_t * max(1, len(labels)))(*[len(x) for x in labels])
    out, size = u8p(), C.c_size_t()
    _check(load_library().apsu_he_wire_build_result_package(bundle_idx, cache_idx, _buf(psu_result), C.c_size_t(len(psu_result)),
                                                            label_byte_count, nonce_byte_count, len(labels), ptrs, sizes,
                                                            C.byref(out), C.byref(size)))
    return _take(out, size)


def parse_result_package(buf):
    """-> dict(bundle_idx, cache_idx, psu_result, label_byte_count, nonce_byte_count, labels)"""
    L = load_library()
    keep = _buf(buf)
    b, c, p, pn, lb, nb, nl = C.c_uint32(), C.c_uint32(), u8p(), C.c_size_t(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(L.apsu_he_wire_parse_result_package(keep, C.c_size_t(len(buf)), C.byref(b), C.byref(c), C.byref(p), C.byref(pn), C.byref(lb),
                                               C.byref(nb), C.byref(nl)))
    labels = []
    for i in range(nl.value):
        q, qn = u8p(), C.c_size_t()
        _check(L.apsu_he_wire_result_label(keep, C.c_size_t(len(buf)), i, C.byref(q), C.byref(qn)))
        labels.append(C.string_at(q, qn.value))
    return dict(bundle_idx=b.value, cache_idx=c.value, psu_result=C.string_at(p, pn.value), label_byte_count=lb.value,
                nonce_byte_count=nb.value, labels=labels)


def seal_ct_save(parms_id, is_ntt_form, ct, correction_factor=1, scale=1.0, version=(4, 0)):
    """UNPINNED envelope (see the header).  ct: uint64 array [size][coeff_modulus_size][n]"""
    import numpy as np
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    pid = (C.c_uint64 * 4)(*parms_id)
    out, size = u8p(), C.c_size_t()
    _check(load_library().apsu_he_wire_seal_ct_save(pid, int(is_ntt_form), C.c_uint64(ct.shape[0]), C.c_uint64(ct.shape[2]),
                                                    C.c_uint64(ct.shape[1]), C.c_uint64(correction_factor), C.c_double(scale),
                                                    ct.ctypes.data_as(C.POINTER(C.c_uint64)), version[0], version[1],
                                                    C.byref(out), C.byref(size)))
    return _take(out, size)


def seal_ct_load(buf):
    import numpy as np
    L = load_library()
    keep = _buf(buf)
    pid = (C.c_uint64 * 4)()
    ntt, sz, n, k, cf, sc, vmaj, vmin = C.c_int(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double(), C.c_int(), C.c_int()
    _check(L.apsu_he_wire_seal_ct_load(keep, C.c_size_t(len(buf)), pid, C.byref(ntt), C.byref(sz), C.byref(n), C.byref(k), C.byref(cf),
                                       C.byref(sc), None, C.c_size_t(0), C.byref(vmaj), C.byref(vmin)))
    data = np.empty((sz.value, k.value, n.value), dtype=np.uint64)
    _check(L.apsu_he_wire_seal_ct_load(keep, C.c_size_t(len(buf)), pid, C.byref(ntt), C.byref(sz), C.byref(n), C.byref(k), C.byref(cf),
                                       C.byref(sc), data.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_size_t(data.size), C.byref(vmaj),
                                       C.byref(vmin)))
    return dict(parms_id=list(pid), is_ntt_form=bool(ntt.value), data=data, correction_factor=cf.value, scale=sc.value,
                version=(vmaj.value, vmin.value))


def bin_bundle_info(buf):
    """one BinBundle as ReceiverDB::save wrote it (bin_bundle.fbs) -> dict(bundle_idx, mod, stripped, n_bins, largest_bin, cache_coeffs, consumed)"""
    keep = _buf(buf)
    bi, nb, lb, cc = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    mod, st, used = C.c_uint64(), C.c_int(), C.c_size_t()
    _check(load_library().apsu_he_wire_bin_bundle_info(keep, C.c_size_t(len(buf)), C.byref(bi), C.byref(mod), C.byref(st), C.byref(nb), C.byref(lb),
                                                      C.byref(cc), C.byref(used)))
    return dict(bundle_idx=bi.value, mod=mod.value, stripped=bool(st.value), n_bins=nb.value, largest_bin=lb.value, cache_coeffs=cc.value,
                consumed=used.value)


def peek_type(buf, is_response=False):
    t = C.c_int()
    _check(load_library().apsu_he_wire_peek_type(_buf(buf), C.c_size_t(len(buf)), 1 if is_response else 0, C.byref(t)))
    return t.value


def psu_params_save(psu_params_json):
    """PSUParams::save: the JSON form -> the binary form (psu_params.fbs + SEAL EncryptionParameters)"""
    out, size = u8p(), C.c_size_t()
    _check(load_library().apsu_he_wire_psu_params_save(psu_params_json.encode(), C.byref(out), C.byref(size)))
    return _take(out, size)


def psu_params_load(buf):
    """PSUParams::Load(binary) -> the JSON text apsu_he_create takes"""
    out, size = u8p(), C.c_size_t()
    _check(load_library().apsu_he_wire_psu_params_load(_buf(buf), C.c_size_t(len(buf)), C.byref(out), C.byref(size)))
    return _take(out, size).decode()


def build_parms_request():
    out, size = u8p(), C.c_size_t()
    _check(load_library().apsu_he_wire_build_parms_request(C.byref(out), C.byref(size)))
    return _take(out, size)


def build_parms_response(psu_params):
    out, size = u8p(), C.c_size_t()
    _check(load_library().apsu_he_wire_build_parms_response(_buf(psu_params), C.c_size_t(len(psu_params)), C.byref(out), C.byref(size)))
    return _take(out, size)


def parse_parms_response(buf):
    keep = _buf(buf)
    p, n = u8p(), C.c_size_t()
    _check(load_library().apsu_he_wire_parse_parms_response(keep, C.c_size_t(len(buf)), C.byref(p), C.byref(n)))
    return C.string_at(p, n.value) if n.value else b""


def build_plain_response(bundle_idx, cache_idx, psu_result):
    import numpy as np
    v = np.ascontiguousarray(psu_result, dtype=np.uint64)
    out, size = u8p(), C.c_size_t()
    _check(load_library().apsu_he_wire_build_plain_response(bundle_idx, cache_idx, v.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_size_t(v.size),
                                                           C.byref(out), C.byref(size)))
    return _take(out, size)


def parse_plain_response(buf):
    import numpy as np
    keep = _buf(buf)
    bi, ci, cnt = C.c_uint32(), C.c_uint32(), C.c_size_t()
    _check(load_library().apsu_he_wire_parse_plain_response(keep, C.c_size_t(len(buf)), C.byref(bi), C.byref(ci), None, C.c_size_t(0), C.byref(cnt)))
    v = np.empty(cnt.value, dtype=np.uint64)
    _check(load_library().apsu_he_wire_parse_plain_response(keep, C.c_size_t(len(buf)), C.byref(bi), C.byref(ci), v.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                           C.c_size_t(v.size), C.byref(cnt)))
    return dict(bundle_idx=bi.value, cache_idx=ci.value, psu_result=v)


def receiver_db_header(buf):
    """the header of a database the reference saved (receiver_db.fbs) -> dict(params_json, item_count, bin_bundle_count, compressed, stripped,
    label_byte_count, consumed)"""
    keep = _buf(buf)
    js, jn = u8p(), C.c_size_t()
    items, bbs, lab, used = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_size_t()
    comp, strip = C.c_int(), C.c_int()
    _check(load_library().apsu_he_wire_receiver_db_header(keep, C.c_size_t(len(buf)), C.byref(js), C.byref(jn), C.byref(items), C.byref(bbs),
                                                         C.byref(comp), C.byref(strip), C.byref(lab), C.byref(used)))
    return dict(params_json=_take(js, jn).decode(), item_count=items.value, bin_bundle_count=bbs.value, compressed=bool(comp.value),
                stripped=bool(strip.value), label_byte_count=lab.value, consumed=used.value)


def saved_size_check(nbytes):
    """the bound every saved-database writer applies before it allocates: raises ApsuHeError naming the size above 2^31 - 1 bytes"""
    _check(load_library().apsu_he_wire_saved_size_check(C.c_uint64(int(nbytes))))


def _ragged(rows):
    """[[felt, ...], ...] -> (flat uint64 array, offsets uint64 array of len(rows) + 1)"""
    import numpy as np
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    if len(rows):
        off[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
    flat = np.array([int(v) for r in rows for v in r], dtype=np.uint64)
    return flat, off


def build_bin_bundle(bundle_idx, mod, item_bins=(), matching_polyns=(), coeffs=(), stripped=False, cache=True):
    """BinBundle::save (bin_bundle.fbs): item_bins / matching_polyns are lists of rows of field elements, coeffs the SEAL-serialised
    plaintexts of cache.batched_matching_polyn; label vectors are written present and empty"""
    u64p = C.POINTER(C.c_uint64)
    bf, bo = _ragged(item_bins)
    pf, po = _ragged(matching_polyns)
    keep = [_buf(c) for c in coeffs]
    ptrs = (C.c_void_p * max(1, len(coeffs)))(*[C.addressof(k) for k in keep])
    sizes = (C.c_size_t * max(1, len(coeffs)))(*[len(c) for c in coeffs])
    out, size = u8p(), C.c_size_t()
    _check(load_library().apsu_he_wire_build_bin_bundle(C.c_uint32(bundle_idx), C.c_uint64(mod), int(bool(stripped)), int(bool(cache)),
                                                        bf.ctypes.data_as(u64p), bo.ctypes.data_as(u64p), C.c_size_t(len(item_bins)),
                                                        pf.ctypes.data_as(u64p), po.ctypes.data_as(u64p), C.c_size_t(len(matching_polyns)),
                                                        ptrs, sizes, C.c_uint32(len(coeffs)), C.byref(out), C.byref(size)))
    return _take(out, size)


def parse_bin_bundle(buf):
    """one saved BinBundle, every field this library reads or writes -> dict(bundle_idx, mod, stripped, has_cache, item_bins,
    matching_polyns (lists of lists), coeffs (list of bytes), label_bins, felt_interp_polyns, batched_interp_polyns (entries of the
    vector, None where it is absent), consumed)"""
    import numpy as np
    L = load_library()
    u64p = C.POINTER(C.c_uint64)
    keep = _buf(buf)
    n = C.c_size_t(len(buf))
    info = bin_bundle_info(buf)

    def rows(which):
        nr, nf = C.c_size_t(), C.c_size_t()
        _check(L.apsu_he_wire_bin_bundle_rows(keep, n, which, None, C.c_size_t(0), None, C.c_size_t(0), C.byref(nr), C.byref(nf)))
        felts, off = np.zeros(max(1, nf.value), dtype=np.uint64), np.zeros(nr.value + 1, dtype=np.uint64)
        _check(L.apsu_he_wire_bin_bundle_rows(keep, n, which, felts.ctypes.data_as(u64p), C.c_size_t(felts.size), off.ctypes.data_as(u64p),
                                              C.c_size_t(off.size), C.byref(nr), C.byref(nf)))
        return [[int(v) for v in felts[int(off[i]):int(off[i + 1])]] for i in range(nr.value)]

    hc, lb, fi, bi = C.c_int(), C.c_int32(), C.c_int32(), C.c_int32()
    _check(L.apsu_he_wire_bin_bundle_extras(keep, n, C.byref(hc), C.byref(lb), C.byref(fi), C.byref(bi)))
    k = info["cache_coeffs"]
    ptrs, sizes, cnt = (u8p * max(1, k))(), (C.c_size_t * max(1, k))(), C.c_uint32()
    _check(L.apsu_he_wire_bin_bundle_coeffs(keep, n, ptrs, sizes, C.c_uint32(k), C.byref(cnt)))
    coeffs = [C.string_at(ptrs[d], sizes[d]) for d in range(cnt.value)]
    opt = lambda v: None if v.value < 0 else v.value
    return dict(bundle_idx=info["bundle_idx"], mod=info["mod"], stripped=info["stripped"], has_cache=bool(hc.value), item_bins=rows(0),
                matching_polyns=rows(1) if hc.value else [], coeffs=coeffs, label_bins=opt(lb), felt_interp_polyns=opt(fi),
                batched_interp_polyns=opt(bi), consumed=info["consumed"])


def build_receiver_db_header(psu_params, item_count=0, bin_bundle_count=0, compressed=False, stripped=False, oprf_key=b"", hashed_items=(),
                             label_byte_count=0, nonce_byte_count=0):
    """ReceiverDB::save's header (receiver_db.fbs): psu_params = psu_params_save's bytes, hashed_items = [(low, high), ...]"""
    import numpy as np
    hi = np.array([[int(a), int(b)] for a, b in hashed_items], dtype=np.uint64).reshape(-1, 2)
    out, size = u8p(), C.c_size_t()
    _check(load_library().apsu_he_wire_build_receiver_db_header(_buf(psu_params), C.c_size_t(len(psu_params)), C.c_uint32(label_byte_count),
                                                                C.c_uint32(nonce_byte_count), C.c_uint64(item_count), int(bool(compressed)),
                                                                int(bool(stripped)), _buf(oprf_key), C.c_size_t(len(oprf_key)),
                                                                hi.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_size_t(hi.shape[0]),
                                                                C.c_uint32(bin_bundle_count), C.byref(out), C.byref(size)))
    return _take(out, size)


def parse_receiver_db_header(buf):
    """receiver_db_header's dict plus psu_params (bytes), oprf_key (bytes), hashed_items ([(low, high)]) and nonce_byte_count"""
    import numpy as np
    keep = _buf(buf)
    d = receiver_db_header(buf)
    pp, pn, kp, kn, hp, hn, nb = u8p(), C.c_size_t(), u8p(), C.c_size_t(), u8p(), C.c_size_t(), C.c_uint32()
    _check(load_library().apsu_he_wire_receiver_db_header_fields(keep, C.c_size_t(len(buf)), C.byref(pp), C.byref(pn), C.byref(kp), C.byref(kn),
                                                                C.byref(hp), C.byref(hn), C.byref(nb)))
    words = np.frombuffer(C.string_at(hp, 16 * hn.value), dtype="<u8").reshape(-1, 2)
    d.update(psu_params=C.string_at(pp, pn.value), oprf_key=C.string_at(kp, kn.value), hashed_items=[(int(a), int(b)) for a, b in words],
             nonce_byte_count=nb.value)
    return d
