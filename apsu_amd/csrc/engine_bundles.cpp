// See engine.h.  The resident database: BinBundles uploaded, generated, built from bins, updated, searched, merged, saved and loaded.
// Where each coefficient of a BinBundle is stored is decided in bundle_layout.h alone; this file shares with the query path
// (engine.cpp) the arena, the streams and the transform launcher (engine_impl.h).
#include "engine_impl.h"

#include <chrono>

#include "seal_codec.h"
#include "wire.h"

namespace apsu_he {

static void bundle_shape(const BundleLayout &y, Bundle &b)
{
    b.degree = y.degree; b.use_ps = y.use_ps; b.H = y.H; b.r = y.r;
    b.pt_level = y.pt_level; b.ntt_count = y.ntt_count;
}

std::unique_ptr<Bundle> Engine::new_bundle(uint32_t bundle_idx, uint32_t cache_idx, uint32_t degree, BundleLayout *layout) const
{
    auto b = std::make_unique<Bundle>();
    b->bundle_idx = bundle_idx;
    b->cache_idx = cache_idx;
    BundleLayout y = layout_of(degree);                          // (refuses ps_low_degree == 1 above degree 1)
    bundle_shape(y, *b);
    if (layout) *layout = std::move(y);
    return b;
}

// bytes of one NTT-form plaintext slot at a level: dense 64-bit words, or bit-packed rows (the same widths as DevLevel::mac_bits)
size_t Engine::slot_bytes(int chain_idx, bool packed) const
{
    const size_t n = hp_.n;
    if (!packed) return (size_t)(chain_idx + 1) * n * sizeof(u64);
    size_t b = 0;
    for (int j = 0; j <= chain_idx; j++) {
        const u32 w = packed_row_bits(hp_.key_q[j]);
        b += n * w / 8;
    }
    return b;
}

void Engine::pack_bundle(Bundle &b)
{
    if (!packed_rows_ || b.packed) return;
    const size_t n = hp_.n;
    const int high = hp_.clamp_chain_idx(1);
    b.ntt_slot_bytes = slot_bytes(b.pt_level, true);
    b.lifted_slot_bytes = slot_bytes(high, true);
    const size_t H = b.lifted.bytes() / ((size_t)(high + 1) * n * sizeof(u64));
    if (b.ntt_count) {
        DevBuf pk;
        pk.alloc(b.ntt_count * b.ntt_slot_bytes + 16);
        HIP_CHECK(hipMemsetAsync(static_cast<char *>(pk.p()) + b.ntt_count * b.ntt_slot_bytes, 0, 16, st_));
        launch_pack_rows(dlevel(b.pt_level), b.pt_level + 1, b.ntt.u(), pk.p(), b.ntt_slot_bytes, n, b.ntt_count, st_);
        sync();
        b.ntt = std::move(pk);
    }
    if (H) {
        DevBuf pk;
        pk.alloc(H * b.lifted_slot_bytes + 16);
        HIP_CHECK(hipMemsetAsync(static_cast<char *>(pk.p()) + H * b.lifted_slot_bytes, 0, 16, st_));
        launch_pack_rows(dlevel(high), high + 1, b.lifted.u(), pk.p(), b.lifted_slot_bytes, n, H, st_);
        sync();
        b.lifted = std::move(pk);
    }
    b.packed = true;
}

void Engine::unpack_bundle(Bundle &b)
{
    if (!b.packed) return;
    const size_t n = hp_.n;
    const int high = hp_.clamp_chain_idx(1);
    if (b.ntt_count) {
        DevBuf dn;
        dn.alloc(b.ntt_count * (size_t)(b.pt_level + 1) * n * sizeof(u64));
        launch_unpack_rows(dlevel(b.pt_level), b.pt_level + 1, b.ntt.p(), b.ntt_slot_bytes, dn.u(), n, b.ntt_count, st_);
        sync();
        b.ntt = std::move(dn);
    }
    const size_t H = b.use_ps ? b.H : 0;
    if (H && b.lifted.bytes()) {
        DevBuf dn;
        dn.alloc(H * (size_t)(high + 1) * n * sizeof(u64));
        launch_unpack_rows(dlevel(high), high + 1, b.lifted.p(), b.lifted_slot_bytes, dn.u(), n, H, st_);
        sync();
        b.lifted = std::move(dn);
    }
    b.packed = false;
    b.ntt_slot_bytes = b.lifted_slot_bytes = 0;
}

std::unique_ptr<Bundle> Engine::upload_bundle(uint32_t bundle_idx, uint32_t cache_idx, uint32_t n_coeffs,
                                              const u64 *const *coeff_ptrs, const unsigned char *is_ntt)
{
    Enter g(this);
    TIER1_SLOTS();
    if (!has_psu_) throw std::logic_error("context was created without PSUParams");
    if (!n_coeffs) throw std::invalid_argument("batched_coeffs is empty");
    if (n_coeffs - 1 > psu_.table_params.max_items_per_bin) throw std::invalid_argument("degree exceeds max_items_per_bin");
    if (bundle_idx >= psu_.bundle_idx_count) throw std::invalid_argument("bundle_idx out of range");
    BundleLayout y;
    auto b = new_bundle(bundle_idx, cache_idx, n_coeffs - 1, &y);
    const size_t n = hp_.n, Lpt = b->pt_level + 1;
    const int high = hp_.clamp_chain_idx(1);
    const size_t Lh = high + 1;
    for (uint32_t i = 0; i < n_coeffs; i++)
        if ((is_ntt[i] != 0) != (y.where(i).kind == COEFF_NTT)) throw std::invalid_argument("plaintext NTT form does not match the BinBundle layout rule");
    b->ntt.alloc(b->ntt_count * Lpt * n * sizeof(u64));
    b->a0.alloc(n * sizeof(u64));
    HIP_CHECK(hipMemcpy(b->a0.p(), coeff_ptrs[0], n * sizeof(u64), hipMemcpyHostToDevice));
    std::vector<unsigned char> mono;
    std::vector<const u64 *> cf;
    for (uint32_t i = 1; i < n_coeffs; i++) {
        if (is_ntt[i]) {
            HIP_CHECK(hipMemcpy(b->ntt.u() + y.where(i).slot * Lpt * n, coeff_ptrs[i], Lpt * n * sizeof(u64), hipMemcpyHostToDevice));
        } else {
            cf.push_back(coeff_ptrs[i]);
            mono.push_back(is_monomial(coeff_ptrs[i], n) ? 1 : 0);
        }
    }
    if (b->use_ps) {
        // K4: pre-lift and pre-NTT the coefficient-form plaintexts a_{i*h} at the high level; this
        // is what multiply_plain (bin_bundle.cpp:334) recomputes on every call in the reference.
        const size_t H = cf.size();
        b->lifted.alloc(H * Lh * n * sizeof(u64));
        WITH_ARENA({
            u64 *raw = ws(H * n);
            unsigned char *flags = ws_as<unsigned char>(H, 1);
            for (size_t i = 0; i < H; i++) H2D(raw + i * n, cf[i], n);
            HIP_CHECK(hipMemcpyAsync(flags, mono.data(), H, hipMemcpyHostToDevice, st_));
            launch_lift(dlevel(high), raw, b->lifted.u(), n, (int)H, flags, st_);
            d_ntt_ct(b->lifted.u(), H, high, false);
            sync();
        });
    }
    pack_bundle(*b);
    return b;
}

// ============================================================================ tier 2: BinBundle construction
// raw = the batched polynomial's coefficient-form plaintexts [degree+1][n] mod t on the device.  Applies the
// layout rule of the BatchedPlaintextPolyn ctor (bin_bundle.cpp:385-420): NTT-form coefficients are lifted
// and transformed at pt_level; coefficient-form a_{i*h} are pre-lifted (honouring SEAL's monomial
// shortcut of multiply_plain) and pre-NTT'd at the high level; a_0 stays raw.
void Engine::finish_bundle(Bundle &b, const u64 *raw)
{
    const uint32_t degree = b.degree;
    const size_t n = hp_.n, Lpt = b.pt_level + 1;
    const int high = hp_.clamp_chain_idx(1);
    const size_t Lh = high + 1;
    b.ntt.alloc(b.ntt_count * Lpt * n * sizeof(u64));
    b.a0.alloc(n * sizeof(u64));
    const size_t H = b.use_ps ? b.H : 0;
    if (H) b.lifted.alloc(H * Lh * n * sizeof(u64));
    D2D(b.a0.u(), raw, n);
    unsigned char *flags = ws_as<unsigned char>(degree + 1, 1);
    launch_flag_monomial(raw, n, (int)degree + 1, flags, st_);
    for (const BundleRun &r : layout_of(degree).runs) {
        if (r.kind == COEFF_NTT) launch_lift(dlevel(b.pt_level), raw + (size_t)r.d0 * n, b.ntt.u() + r.first_slot * Lpt * n, n, (int)r.count, nullptr, st_);
        else if (H) launch_lift(dlevel(high), raw + (size_t)r.d0 * n, b.lifted.u() + r.first_slot * Lh * n, n, (int)r.count, flags + r.d0, st_);
    }
    d_ntt_ct(b.ntt.u(), b.ntt_count, b.pt_level, false);
    if (H) d_ntt_ct(b.lifted.u(), H, high, false);
}

std::unique_ptr<Bundle> Engine::random_bundle(uint32_t bundle_idx, uint32_t cache_idx, uint32_t degree, u64 seed)
{
    Enter g(this);
    TIER1_SLOTS();
    if (!has_psu_) throw std::logic_error("context was created without PSUParams");
    if (degree > psu_.table_params.max_items_per_bin) throw std::invalid_argument("degree exceeds max_items_per_bin");
    auto b = new_bundle(bundle_idx, cache_idx, degree);
    const size_t n = hp_.n;
    // coefficient d, index k of the batched polynomial = splitmix64 stream at offset d*n + k (mod t), coefficient form
    WITH_ARENA({
        u64 *raw = ws((size_t)(degree + 1) * n);
        launch_fill_random(raw, (size_t)(degree + 1) * n, seed, hp_.t, st_);
        finish_bundle(*b, raw);
        sync();
    });
    pack_bundle(*b);
    return b;
}

std::unique_ptr<Bundle> Engine::build_bundle(uint32_t bundle_idx, uint32_t cache_idx, const u64 *roots, const uint32_t *counts,
                                             uint32_t bins, uint32_t stride)
{
    Enter g(this);
    TIER1_SLOTS();
    if (!has_psu_) throw std::logic_error("context was created without PSUParams");
    if (!hp_.batching) throw std::logic_error("plain_modulus does not support batching");
    const size_t n = hp_.n;
    if (bins > n) throw std::invalid_argument("more bins than batching slots");
    if (bundle_idx >= psu_.bundle_idx_count) throw std::invalid_argument("bundle_idx out of range");
    uint32_t degree = 0;
    for (uint32_t s = 0; s < bins; s++) {
        if (counts[s] > stride) throw std::invalid_argument("bin count exceeds stride");
        degree = std::max(degree, counts[s]);
    }
    // a bin may hold at most max_items_per_bin - 1 items (receiver_db.cpp:388-389: insertion requires size < max)
    if (degree > psu_.table_params.max_items_per_bin) throw std::invalid_argument("bin size exceeds max_items_per_bin");
    for (uint32_t s = 0; s < bins; s++)
        for (uint32_t r = 0; r < counts[s]; r++)
            if (roots[(size_t)s * stride + r] >= hp_.t) throw std::invalid_argument("field element is not reduced modulo plain_modulus");
    auto b = new_bundle(bundle_idx, cache_idx, degree);
    WITH_ARENA({
        u64 *droots = ws((size_t)bins * stride + 1);
        uint32_t *dcounts = ws_as<uint32_t>(bins, 1);
        if (bins) {
            H2D(droots, roots, (size_t)bins * stride);
            HIP_CHECK(hipMemcpyAsync(dcounts, counts, bins * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
        }
        u64 *poly = ws((size_t)(degree + 1) * n);                  // [d][slot] slot values of the batched polynomial
        launch_polyn_with_roots(droots, dcounts, bins, stride, degree, make_mod(hp_.t), poly, n, st_);
        encode_bundle(*b, poly);
        sync();
    });
    pack_bundle(*b);
    return b;
}

// the tail of build_bundle and update_bundle: slot values [degree+1][n] of the batched polynomial -> the stored BinBundle
void Engine::encode_bundle(Bundle &b, const u64 *poly)
{
    const size_t n = hp_.n;
    // BatchEncoder::encode (bin_bundle.cpp:409): slot permutation, then inverse negacyclic NTT mod t
    u64 *raw = ws((size_t)(b.degree + 1) * n);
    launch_scatter_slots(poly, reinterpret_cast<const uint32_t *>(d_slot_map_.p()), raw, n, (int)b.degree + 1, st_);
    d_ntt(raw, b.degree + 1, map_ct() + hp_.plain_id(), 1, true, false);
    finish_bundle(b, raw);
}

// The inverse of encode_bundle, whoever made the BinBundle: coefficient d -> its stored form as in finish_bundle (a_0 raw; NTT-form
// rows and the pre-lifted a_{i h}: limb 0, the residues mod q_0), inverse NTT over q_0, un-lift (bin_update.h; SEAL's un-lifted
// monomials included), forward NTT mod t, slot gather -- BatchEncoder::decode.
void Engine::decode_bundle(const Bundle &b, u64 *poly, u64 *coeff)
{
    const uint32_t degree = b.degree;
    const size_t n = hp_.n, Lpt = b.pt_level + 1;
    const int high = hp_.clamp_chain_idx(1);
    const size_t Lh = high + 1;
    u64 *raw = ws((size_t)(degree + 1) * n);
    D2D(raw, b.a0.u(), n);
    for (const BundleRun &r : layout_of(degree).runs) {                  // the runs finish_bundle wrote
        const bool ntt = r.kind == COEFF_NTT;
        if (!ntt && !b.use_ps) throw std::logic_error("BinBundle holds a coefficient-form plaintext it cannot evaluate");
        const size_t L = ntt ? Lpt : Lh, sb = !b.packed ? L * n * sizeof(u64) : ntt ? b.ntt_slot_bytes : b.lifted_slot_bytes;
        launch_limb0_rows(dlevel(ntt ? b.pt_level : high), (int)L, static_cast<const char *>((ntt ? b.ntt : b.lifted).p()) + r.first_slot * sb, sb, b.packed,
                          raw + (size_t)r.d0 * n, n, r.count, st_);
    }
    if (degree) {
        d_ntt(raw + n, degree, map_ct(), 1, true, data_primes_narrow_);
        launch_unlift(raw + n, (size_t)degree * n, hp_.t, hp_.key_q[0], st_);
    }
    if (coeff) D2D(coeff, raw, (size_t)(degree + 1) * n);
    d_ntt(raw, degree + 1, map_ct() + hp_.plain_id(), 1, false, false);
    launch_gather_slots(raw, reinterpret_cast<const uint32_t *>(d_slot_map_.p()), poly, n, (int)degree + 1, st_);
}

std::unique_ptr<Bundle> Engine::update_bundle(const Bundle &old, const u64 *ins_roots, const uint32_t *ins_counts, uint32_t ins_stride,
                                              const u64 *rem_roots, const uint32_t *rem_counts, uint32_t rem_stride, uint32_t bins)
{
    Enter g(this);
    TIER1_SLOTS();
    if (!has_psu_) throw std::logic_error("context was created without PSUParams");
    if (!hp_.batching) throw std::logic_error("plain_modulus does not support batching");
    if (!unlift_exact_) throw std::logic_error("q_0 <= 2 * plain_modulus: stored plaintexts cannot be decoded");
    const size_t n = hp_.n;
    if (bins > n) throw std::invalid_argument("more bins than batching slots");
    if ((ins_roots == nullptr) != (ins_counts == nullptr) || (rem_roots == nullptr) != (rem_counts == nullptr))
        throw std::invalid_argument("a root list and its counts are given together or not at all");
    const uint32_t max_items = psu_.table_params.max_items_per_bin;
    std::vector<uint32_t> touched;
    uint32_t max_ins = 0;
    for (uint32_t s = 0; s < bins; s++) {
        const uint32_t ni = ins_counts ? ins_counts[s] : 0, nr = rem_counts ? rem_counts[s] : 0;
        if (ni > ins_stride || nr > rem_stride) throw std::invalid_argument("bin count exceeds stride");
        if (ni > max_items) throw std::invalid_argument("bin size exceeds max_items_per_bin");
        for (uint32_t r = 0; r < ni; r++)
            if (ins_roots[(size_t)s * ins_stride + r] >= hp_.t) throw std::invalid_argument("field element is not reduced modulo plain_modulus");
        for (uint32_t r = 0; r < nr; r++)
            if (rem_roots[(size_t)s * rem_stride + r] >= hp_.t) throw std::invalid_argument("field element is not reduced modulo plain_modulus");
        max_ins = std::max(max_ins, ni);
        if (ni || nr) touched.push_back(s);
    }
    const uint32_t rows = old.degree + max_ins + 1;                    // no bin can outgrow this
    const size_t ins_words = ins_counts ? (size_t)bins * ins_stride : 0, rem_words = rem_counts ? (size_t)bins * rem_stride : 0;
    std::unique_ptr<Bundle> b;
    WITH_ARENA({
        u64 *poly = ws((size_t)rows * n);                              // [d][slot] slot values of the batched polynomial
        decode_bundle(old, poly);
        if (rows > old.degree + 1) HIP_CHECK(hipMemsetAsync(poly + (size_t)(old.degree + 1) * n, 0, (size_t)(rows - old.degree - 1) * n * sizeof(u64), st_));
        u64 *status = ws(3);                                           // failed removal, unused slot named (both atomicMin), degree (atomicMax)
        HIP_CHECK(hipMemsetAsync(status, 0xff, 2 * sizeof(u64), st_));
        HIP_CHECK(hipMemsetAsync(status + 2, 0, sizeof(u64), st_));
        std::vector<uint32_t> new_counts(touched.size());
        if (!touched.empty()) {
            u64 *dins = ws(ins_words + 1), *drem = ws(rem_words + 1);
            uint32_t *dic = ws_as<uint32_t>(bins, 1), *drc = ws_as<uint32_t>(bins, 1);
            uint32_t *dtouched = ws_as<uint32_t>(touched.size(), 1), *dnew = ws_as<uint32_t>(touched.size(), 1);
            if (ins_words) H2D(dins, ins_roots, ins_words);
            if (rem_words) H2D(drem, rem_roots, rem_words);
            if (ins_counts) HIP_CHECK(hipMemcpyAsync(dic, ins_counts, bins * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
            if (rem_counts) HIP_CHECK(hipMemcpyAsync(drc, rem_counts, bins * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
            HIP_CHECK(hipMemcpyAsync(dtouched, touched.data(), touched.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
            launch_bins_update(dtouched, (u32)touched.size(), dins, ins_counts ? dic : nullptr, ins_stride, drem, rem_counts ? drc : nullptr, rem_stride,
                               make_mod(hp_.t), poly, n, rows, dnew, status, st_);
            HIP_CHECK(hipMemcpyAsync(new_counts.data(), dnew, touched.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
        }
        launch_poly_degree(poly, n, rows, status + 2, st_);
        u64 st[3];
        HIP_CHECK(hipMemcpyAsync(st, status, sizeof(st), hipMemcpyDeviceToHost, st_));
        sync();                                                        // the new shape is decided on the host
        if (st[1] != ~(u64)0)
            throw std::invalid_argument("bin " + std::to_string(st[1]) + " is an unused slot (it holds the zero polynomial): nothing can be inserted or removed there");
        if (st[0] != ~(u64)0) {
            const uint32_t s = (uint32_t)(st[0] >> 32), r = (uint32_t)st[0];
            throw std::invalid_argument("bin " + std::to_string(s) + ": " + std::to_string(rem_roots[(size_t)s * rem_stride + r]) + " (removal " +
                                        std::to_string(r) + ") is not a root of the bin's polynomial");
        }
        uint32_t degree = (uint32_t)st[2];                             // untouched bins included (k_poly_degree)
        for (uint32_t c : new_counts) degree = std::max(degree, c);
        if (degree > max_items) throw std::invalid_argument("bin size exceeds max_items_per_bin");
        b = new_bundle(old.bundle_idx, old.cache_idx, degree);
        encode_bundle(*b, poly);
        sync();
    });
    pack_bundle(*b);
    return b;
}

void EventStamps::reserve(size_t count)
{
    while (ev.size() < count) {
        hipEvent_t e;
        HIP_CHECK(hipEventCreate(&e));
        ev.push_back(e);
    }
}
void EventStamps::record(size_t i, hipStream_t st) { HIP_CHECK(hipEventRecord(ev.at(i), st)); }
double EventStamps::ms(size_t from, size_t to) const
{
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, ev[from], ev[to]));
    return ms;
}
void EventStamps::release()
{
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    ev.clear();
}

// ---- N1, find and place: occupancy, membership and the database-level step on resident BinBundles
void Engine::lookup_check(const char *what) const
{
    if (!has_psu_) throw std::logic_error("context was created without PSUParams");
    if (!hp_.batching) throw std::logic_error("plain_modulus does not support batching");
    if (!unlift_exact_) throw std::logic_error("q_0 <= 2 * plain_modulus: stored plaintexts cannot be decoded");
    if (psu_.bins_per_bundle > hp_.n) throw std::logic_error(std::string(what) + ": more bins than batching slots");
}

void Engine::lookup_impl(const Bundle *const *bundles, uint32_t n_bundles, const u64 *felts, const uint32_t *start, size_t count, uint32_t *counts,
                         unsigned char *flags)
{
    const size_t n = hp_.n;
    const uint32_t F = psu_.item_params.felts_per_item;
    if (count && count >= (size_t)LOOKUP_NONE / F) throw std::invalid_argument("too many entries for one call");
    for (size_t e = 0; e < count; e++) {
        if ((u64)start[e] + F > psu_.bins_per_bundle) throw std::invalid_argument("entry " + std::to_string(e) + ": start bin + felts_per_item exceeds bins_per_bundle");
        for (uint32_t j = 0; j < F; j++)
            if (felts[e * F + j] >= hp_.t) throw std::invalid_argument("entry " + std::to_string(e) + ": field element is not reduced modulo plain_modulus");
    }
    const size_t parts = count * F;
    const LookupPlan plan = count ? lookup_plan(felts, start, count, F, n, LOOKUP_R) : LookupPlan();
    lookup_evs_.reserve((size_t)3 * n_bundles);
    WITH_ARENA({
        LookupWork *dwork = nullptr;
        u64 *dpts = nullptr;
        uint32_t *didx = nullptr;
        if (count) {
            dwork = ws_as<LookupWork>(plan.work.size());
            dpts = ws(plan.pts.size());
            didx = ws_as<uint32_t>(plan.idx.size());
            HIP_CHECK(hipMemcpyAsync(dwork, plan.work.data(), plan.work.size() * sizeof(LookupWork), hipMemcpyHostToDevice, st_));
            HIP_CHECK(hipMemcpyAsync(dpts, plan.pts.data(), plan.pts.size() * sizeof(u64), hipMemcpyHostToDevice, st_));
            HIP_CHECK(hipMemcpyAsync(didx, plan.idx.data(), plan.idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
        }
        unsigned char *dflags = count ? ws_as<unsigned char>(parts) : nullptr;
        uint32_t *dcounts = counts ? ws_as<uint32_t>(n) : nullptr;
        const size_t mark = arena_off_;
        for (uint32_t i = 0; i < n_bundles; i++) {
            const Bundle &b = *bundles[i];
            arena_off_ = mark;                                         // one BinBundle after the other through the same workspace (stream order)
            lookup_evs_.record(3 * i, st_);
            u64 *poly = ws((size_t)(b.degree + 1) * n);                // [d][slot] slot values of the batched polynomial
            decode_bundle(b, poly);
            lookup_evs_.record(3 * i + 1, st_);
            if (counts) {
                launch_bin_counts(poly, n, b.degree + 1, dcounts, st_);
                HIP_CHECK(hipMemcpyAsync(counts + (size_t)i * n, dcounts, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
            }
            if (count) {
                launch_bins_lookup(dwork, (u32)plan.work.size(), dpts, didx, make_mod(hp_.t), poly, n, b.degree, dflags, st_);
                HIP_CHECK(hipMemcpyAsync(flags + (size_t)i * parts, dflags, parts, hipMemcpyDeviceToHost, st_));
            }
            lookup_evs_.record(3 * i + 2, st_);
        }
        sync();
    });
    lookup_decode_ms_ = lookup_kernels_ms_ = 0;
    for (uint32_t i = 0; i < n_bundles; i++) {
        lookup_decode_ms_ += lookup_evs_.ms(3 * i, 3 * i + 1);
        lookup_kernels_ms_ += lookup_evs_.ms(3 * i + 1, 3 * i + 2);
    }
}

void Engine::lookup_times(double *decode_ms, double *kernels_ms)
{
    Enter g(this);
    if (decode_ms) *decode_ms = lookup_decode_ms_;
    if (kernels_ms) *kernels_ms = lookup_kernels_ms_;
}

void Engine::bin_counts(const Bundle &b, uint32_t *counts)
{
    Enter g(this);
    TIER1_SLOTS();
    lookup_check("bin_counts");
    const Bundle *one = &b;
    lookup_impl(&one, 1, nullptr, nullptr, 0, counts, nullptr);
}

// present[b][e] = AND over the entry's parts; room[b][e] = max_j(count[s + j] + 1), multi_insert_dry_run's return value, or LOOKUP_NONE
static void lookup_reduce(const unsigned char *flags, const uint32_t *counts, uint32_t n_bundles, size_t n, const uint32_t *start, size_t count, uint32_t F,
                          unsigned char *present, uint32_t *room)
{
    for (uint32_t b = 0; b < n_bundles; b++)
        for (size_t e = 0; e < count; e++) {
            unsigned char all = 1;
            uint32_t most = 0;
            for (uint32_t j = 0; j < F; j++) {
                all &= flags[((size_t)b * count + e) * F + j];
                const uint32_t c = counts[(size_t)b * n + start[e] + j];
                most = most == LOOKUP_NONE || c == LOOKUP_NONE ? LOOKUP_NONE : std::max(most, c + 1);
            }
            if (present) present[(size_t)b * count + e] = all;
            if (room) room[(size_t)b * count + e] = most;
        }
}

void Engine::lookup_bundles(const Bundle *const *bundles, uint32_t n_bundles, const u64 *felts, const uint32_t *start, size_t count,
                            unsigned char *present, uint32_t *room)
{
    Enter g(this);
    TIER1_SLOTS();
    lookup_check("lookup");
    if (!n_bundles || !count) return;
    const size_t n = hp_.n;
    const uint32_t F = psu_.item_params.felts_per_item;
    std::vector<unsigned char> flags((size_t)n_bundles * count * F);
    std::vector<uint32_t> counts((size_t)n_bundles * n);
    lookup_impl(bundles, n_bundles, felts, start, count, counts.data(), flags.data());
    lookup_reduce(flags.data(), counts.data(), n_bundles, n, start, count, F, present, room);
}

// ---- N1, reading the bins back (bin_roots.h): decode, k_bin_counts, k_bin_roots (or the per-coset composition), k_roots_mult, one sync,
// then the host's sort per bin and the sum check
void Engine::roots_tables()
{
    if (roots_g_) return;
    const size_t n = hp_.n;
    const u64 g = field_generator(hp_.t);
    const std::vector<u32> step = roots_step_table(g, hp_.t, n);
    d_roots_step_.alloc(n * sizeof(u32));
    HIP_CHECK(hipMemcpy(d_roots_step_.p(), step.data(), n * sizeof(u32), hipMemcpyHostToDevice));
    // the evaluation point of output position k is the transform of X at k: the output order is the launch's own
    d_roots_pts_.alloc(n * sizeof(u64));
    std::vector<u64> x(n, 0);
    x[1] = 1;
    HIP_CHECK(hipMemcpy(d_roots_pts_.p(), x.data(), n * sizeof(u64), hipMemcpyHostToDevice));
    d_ntt(d_roots_pts_.u(), 1, map_ct() + hp_.plain_id(), 1, false, false);
    sync();
    roots_g_ = g;
}

void Engine::bundle_bins(const Bundle &b, u64 *roots, uint32_t *counts, uint32_t stride, int form)
{
    Enter g(this);
    TIER1_SLOTS();
    bins_impl(b, roots, counts, stride, form, nullptr);
}

void Engine::bins_impl(const Bundle &b, u64 *roots, uint32_t *counts, uint32_t stride, int form, BinsTap *tap)
{
    lookup_check("bins");
    const size_t n = hp_.n;
    const u32 cosets = roots_coset_count(hp_.t, n);                    // (refuses a plain modulus with too many cosets)
    if (b.degree >= n) throw std::logic_error("bins: a bin's polynomial of degree " + std::to_string(b.degree) + " does not fit one transform of " + std::to_string(n) + " points");
    const bool has_kernel = bin_roots_has_kernel(hp_.logn);
    if (form == BINS_FORM_KERNEL && !has_kernel) throw std::logic_error("bins: no persistent kernel for this ring size");
    const bool kernel = form == BINS_FORM_COMPOSED ? false : has_kernel;
    roots_tables();
    const Mod t = make_mod(hp_.t);
    const u32 *step = reinterpret_cast<const u32 *>(d_roots_step_.p());
    const u64 *pts = d_roots_pts_.u();
    std::vector<uint32_t> occ;
    std::vector<u64> hits;
    std::vector<uint32_t> found, mult;
    uint32_t hstride = 0;
    bins_evs_.reserve(4);
    WITH_ARENA({
        occ.clear();
        hstride = 0;
        bins_evs_.record(0, st_);
        u64 *poly = ws((size_t)(b.degree + 1) * n);                    // [d][slot] slot values of the batched polynomial
        uint32_t *dcounts = ws_as<uint32_t>(n);
        u64 *coeff = tap ? ws((size_t)(b.degree + 1) * n) : nullptr;
        const size_t mark = arena_off_;
        decode_bundle(b, poly, coeff);
        arena_off_ = mark;                                             // the decode's workspace is free again (stream order)
        launch_bin_counts(poly, n, b.degree + 1, dcounts, st_);
        HIP_CHECK(hipMemcpyAsync(counts, dcounts, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
        bins_evs_.record(1, st_);
        sync();                                                        // which bins are occupied, and the lists' size, are decided on the host
        if (tap) tap->after_counts(poly, coeff, dcounts, counts);
        for (size_t s = 0; s < n; s++)
            if (counts[s] != LOOKUP_NONE && counts[s] >= 1) { occ.push_back((uint32_t)s); hstride = std::max(hstride, counts[s]); }
        if (roots && stride < hstride) throw std::invalid_argument("bins: stride " + std::to_string(stride) + " is below the largest bin count " + std::to_string(hstride));
        const u32 n_occ = (u32)occ.size();
        if (n_occ) {
            uint32_t *docc = ws_as<uint32_t>(n_occ), *dfound = ws_as<uint32_t>(n_occ), *dmult = ws_as<uint32_t>((size_t)n_occ * hstride);
            u64 *dhits = ws((size_t)n_occ * hstride);
            HIP_CHECK(hipMemcpyAsync(docc, occ.data(), n_occ * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
            HIP_CHECK(hipMemsetAsync(dfound, 0, n_occ * sizeof(uint32_t), st_));
            if (kernel) {
                const u32 slots = bin_roots_wg_slots(hp_.logn);
                const RootsGrid grid = roots_grid(n_occ, cosets, slots);
                const u32 wgs = (u32)std::min<u64>((u64)n_occ * grid.blocks, slots);
                u64 *rows = ws((size_t)wgs * n);
                u32 *vrows = ws_as<u32>((size_t)wgs * n);
                launch_bin_roots(hp_.logn, poly, docc, dcounts, n_occ, grid, cosets, wgs, tabs(), map_ct() + hp_.plain_id(), step, pts, roots_g_, rows, vrows,
                                 dhits, dfound, hstride, st_);
            } else {
                // limb rows of at most 64 MiB at a time, all cosets for one group of bins, then the next group
                const u32 group = (u32)std::max<size_t>(1, std::min<size_t>(n_occ, ((size_t)64 << 20) / (n * sizeof(u64))));
                u64 *rows = ws((size_t)group * n);
                const u64 r1 = t.r1;
                for (u32 r0 = 0; r0 < n_occ; r0 += group) {
                    const u32 nr = std::min(group, n_occ - r0);
                    u64 c = 1;
                    for (u32 j = 0; j < cosets; j++) {
                        launch_roots_gather(poly, n, docc + r0, dcounts, nr, c, t, rows, st_);
                        d_ntt(rows, nr, map_ct() + hp_.plain_id(), 1, false, false);
                        launch_roots_scan(rows, n, nr, pts, c, t, j == 0, poly, docc + r0, dcounts, dhits + (size_t)r0 * hstride, dfound + r0, hstride, st_);
                        c = roots_mul(c, roots_g_, hp_.t, r1);
                    }
                }
            }
            bins_evs_.record(2, st_);
            launch_roots_mult(poly, n, docc, dcounts, n_occ, t, dhits, dfound, dmult, hstride, st_);
            hits.resize((size_t)n_occ * hstride); found.resize(n_occ); mult.resize((size_t)n_occ * hstride);
            HIP_CHECK(hipMemcpyAsync(found.data(), dfound, n_occ * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
            HIP_CHECK(hipMemcpyAsync(mult.data(), dmult, mult.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
            HIP_CHECK(hipMemcpyAsync(hits.data(), dhits, hits.size() * sizeof(u64), hipMemcpyDeviceToHost, st_));
        } else bins_evs_.record(2, st_);
        bins_evs_.record(3, st_);
        sync();
    });
    for (int i = 0; i < 3; i++) bins_ms_[i] = bins_evs_.ms(i, i + 1);
    // host end: multiplicities (1 wherever a bin has as many distinct roots as items), the sum check, the sort; nothing is written to
    // `roots` before every bin has passed
    std::vector<std::vector<u64>> bins(occ.size());
    for (size_t r = 0; r < occ.size(); r++) {
        const u32 cnt = counts[occ[r]], nf = found[r];
        u32 *m = mult.data() + r * hstride;
        if (nf >= cnt) std::fill(m, m + std::min(nf, cnt), 1u);
        roots_expand(occ[r], cnt, hits.data() + r * hstride, m, nf, bins[r]);
    }
    if (!roots) return;
    for (size_t r = 0; r < occ.size(); r++) std::copy(bins[r].begin(), bins[r].end(), roots + (size_t)occ[r] * stride);
}

void Engine::bins_times(double *decode_ms, double *roots_ms, double *mult_ms)
{
    Enter g(this);
    if (decode_ms) *decode_ms = bins_ms_[0];
    if (roots_ms) *roots_ms = bins_ms_[1];
    if (mult_ms) *mult_ms = bins_ms_[2];
}

// apply_entries and compact take the BinBundles of one bundle index, in cache order
static void check_one_index_in_cache_order(uint32_t bundle_idx, const Bundle *const *bundles, uint32_t n_bundles)
{
    for (uint32_t b = 0; b < n_bundles; b++) {
        if (bundles[b]->bundle_idx != bundle_idx) throw std::invalid_argument("the BinBundles of one call belong to one bundle index");
        if (b && bundles[b]->cache_idx <= bundles[b - 1]->cache_idx) throw std::invalid_argument("BinBundles are not in cache order");
    }
}

PlaceResult place_from_lookup(uint32_t n_bundles, size_t n, uint32_t bins, uint32_t F, uint32_t max_items, u64 t, const uint32_t *counts,
                              const unsigned char *present, const u64 *ins_felts, const uint32_t *ins_start, size_t n_ins, const u64 *rem_felts,
                              const uint32_t *rem_start, size_t n_rem)
{
    const size_t count = n_rem + n_ins;
    std::vector<uint32_t> bin_counts((size_t)n_bundles * bins);
    std::vector<unsigned char> ins_present((size_t)n_bundles * n_ins), rem_present((size_t)n_bundles * n_rem);
    for (uint32_t b = 0; b < n_bundles; b++) {
        std::copy(counts + (size_t)b * n, counts + (size_t)b * n + bins, bin_counts.begin() + (size_t)b * bins);
        std::copy(present + (size_t)b * count, present + (size_t)b * count + n_rem, rem_present.begin() + (size_t)b * n_rem);
        std::copy(present + (size_t)b * count + n_rem, present + (size_t)(b + 1) * count, ins_present.begin() + (size_t)b * n_ins);
    }
    PlaceInput in;
    in.n_bundles = n_bundles; in.bins = bins; in.F = F; in.max_items = max_items; in.t = t;
    in.counts = bin_counts.data(); in.ins_present = ins_present.data(); in.rem_present = rem_present.data();
    in.ins_felts = ins_felts; in.ins_start = ins_start; in.n_ins = n_ins;
    in.rem_felts = rem_felts; in.rem_start = rem_start; in.n_rem = n_rem;
    return place_entries(in);
}

void Engine::lookup_counts(const char *what, const Bundle *const *bundles, uint32_t n_bundles, const u64 *felts, const uint32_t *start, size_t count,
                           uint32_t *counts, unsigned char *present)
{
    Enter g(this);
    TIER1_SLOTS();
    lookup_check(what);
    if (!n_bundles) return;
    const size_t n = hp_.n;
    const uint32_t F = psu_.item_params.felts_per_item;
    std::vector<unsigned char> flags((size_t)n_bundles * count * F);
    lookup_impl(bundles, n_bundles, felts, start, count, counts, count ? flags.data() : nullptr);
    if (count) lookup_reduce(flags.data(), counts, n_bundles, n, start, count, F, present, nullptr);
}

std::unique_ptr<Bundle> Engine::clone_bundle(const Bundle &src, int src_device)
{
    Enter g(this);
    if (!has_psu_) throw std::logic_error("context was created without PSUParams");
    if (src.packed != packed_rows_) throw std::logic_error("the BinBundle's rows are in the other format (APSU_HE_PACKED_ROWS differs between the contexts)");
    auto b = new_bundle(src.bundle_idx, src.cache_idx, src.degree);
    if (b->ntt_count != src.ntt_count || b->pt_level != src.pt_level || b->use_ps != src.use_ps || b->H != src.H)
        throw std::invalid_argument("BinBundle was made for different parameters");
    b->packed = src.packed; b->ntt_slot_bytes = src.ntt_slot_bytes; b->lifted_slot_bytes = src.lifted_slot_bytes;
    const DevBuf *from[3] = { &src.ntt, &src.lifted, &src.a0 };
    DevBuf *to[3] = { &b->ntt, &b->lifted, &b->a0 };
    for (int i = 0; i < 3; i++) {
        if (!from[i]->bytes()) continue;
        to[i]->alloc(from[i]->bytes());
        // (a handle may list one device twice: two contexts, one device, an ordinary copy)
        if (src_device == device_) HIP_CHECK(hipMemcpyAsync(to[i]->p(), from[i]->p(), from[i]->bytes(), hipMemcpyDeviceToDevice, st_));
        else HIP_CHECK(hipMemcpyPeerAsync(to[i]->p(), device_, from[i]->p(), src_device, from[i]->bytes(), st_));
    }
    sync();
    return b;
}

Engine::ApplyResult Engine::apply_entries(uint32_t bundle_idx, const Bundle *const *bundles, uint32_t n_bundles, const u64 *ins_felts,
                                          const uint32_t *ins_start, size_t n_ins, const u64 *rem_felts, const uint32_t *rem_start, size_t n_rem)
{
    ApplyResult res;
    const size_t n = hp_.n;
    uint32_t F = 0, bins = 0;
    std::vector<uint32_t> counts;
    {
        Enter g(this);
        TIER1_SLOTS();
        lookup_check("apply_entries");
        F = psu_.item_params.felts_per_item;
        bins = psu_.bins_per_bundle;
        if (bundle_idx >= psu_.bundle_idx_count) throw std::invalid_argument("bundle_idx out of range");
        check_one_index_in_cache_order(bundle_idx, bundles, n_bundles);
        // the refusals come before any GPU work
        place_validate(ins_felts, ins_start, n_ins, rem_felts, rem_start, n_rem, F, bins, hp_.t);
        // one lookup for both lists: removals first, insertions behind them
        std::vector<u64> felts((n_rem + n_ins) * F);
        std::vector<uint32_t> start(n_rem + n_ins);
        std::copy(rem_felts, rem_felts + n_rem * F, felts.begin());
        std::copy(ins_felts, ins_felts + n_ins * F, felts.begin() + n_rem * F);
        std::copy(rem_start, rem_start + n_rem, start.begin());
        std::copy(ins_start, ins_start + n_ins, start.begin() + n_rem);
        const size_t count = n_rem + n_ins;
        std::vector<unsigned char> flags((size_t)n_bundles * count * F), present((size_t)n_bundles * count);
        counts.assign((size_t)n_bundles * n, 0);
        if (n_bundles) {
            lookup_impl(bundles, n_bundles, felts.data(), start.data(), count, counts.data(), count ? flags.data() : nullptr);
            lookup_reduce(flags.data(), counts.data(), n_bundles, n, start.data(), count, F, present.data(), nullptr);
        }
        res.place = place_from_lookup(n_bundles, n, bins, F, psu_.table_params.max_items_per_bin, hp_.t, counts.data(), present.data(), ins_felts,
                                      ins_start, n_ins, rem_felts, rem_start, n_rem);
    }
    // the context's lock is taken per step from here on, as by a caller who made these calls one by one; the given BinBundles are only read
    const PlaceResult &pl = res.place;
    res.replaced.resize(n_bundles);
    for (uint32_t b = 0; b < n_bundles; b++) {
        if (pl.state[b] != PLACE_REPLACED) continue;
        const PlaceLists &li = pl.ins[b], &lr = pl.rem[b];
        res.replaced[b] = update_bundle(*bundles[b], li.any() ? li.roots.data() : nullptr, li.any() ? li.counts.data() : nullptr, li.stride,
                                        lr.any() ? lr.roots.data() : nullptr, lr.any() ? lr.counts.data() : nullptr, lr.stride, bins);
    }
    const uint32_t next_cache = n_bundles ? bundles[n_bundles - 1]->cache_idx + 1 : 0;
    for (uint32_t k = 0; k < pl.n_new; k++) {
        const PlaceLists &li = pl.ins[n_bundles + k];
        res.appended.push_back(build_bundle(bundle_idx, next_cache + k, li.roots.data(), li.counts.data(), bins, li.stride));
    }
    return res;
}

// ---- N1, compaction: several BinBundles of one bundle index into one (bin_merge.h, db_compact.h)
std::unique_ptr<Bundle> Engine::merge_bundles(const Bundle *const *bundles, uint32_t n_bundles, uint32_t cache_idx)
{
    Enter g(this);
    TIER1_SLOTS();
    lookup_check("merge");
    if (n_bundles < 2) throw std::invalid_argument("a merge takes at least two BinBundles");
    for (uint32_t i = 1; i < n_bundles; i++)
        if (bundles[i]->bundle_idx != bundles[0]->bundle_idx)
            throw std::invalid_argument("BinBundle " + std::to_string(i) + " belongs to bundle index " + std::to_string(bundles[i]->bundle_idx) +
                                        ", the first to " + std::to_string(bundles[0]->bundle_idx));
    const size_t n = hp_.n, tiles = (n + MERGE_LANES - 1) / MERGE_LANES;
    const uint32_t max_items = psu_.table_params.max_items_per_bin;
    std::unique_ptr<Bundle> b;
    merge_evs_.reserve(5);
    WITH_ARENA({
        merge_evs_.record(0, st_);
        std::vector<u64 *> poly(n_bundles);
        for (uint32_t i = 0; i < n_bundles; i++) poly[i] = ws((size_t)(bundles[i]->degree + 1) * n);       // [d][slot] slot values
        uint32_t *dcounts = ws_as<uint32_t>((size_t)n_bundles * n);
        const size_t mark = arena_off_;
        for (uint32_t i = 0; i < n_bundles; i++) {
            arena_off_ = mark;                                         // the decodes share their workspace (stream order)
            decode_bundle(*bundles[i], poly[i]);
            launch_bin_counts(poly[i], n, bundles[i]->degree + 1, dcounts + (size_t)i * n, st_);
        }
        arena_off_ = mark;
        std::vector<uint32_t> counts((size_t)n_bundles * n);
        HIP_CHECK(hipMemcpyAsync(counts.data(), dcounts, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
        merge_evs_.record(1, st_);
        sync();                                                        // what may be merged, and every step's shape, is decided on the host
        // step k multiplies the product of BinBundles 0 .. k by BinBundle k + 1; every refusal comes before the first product
        const uint32_t steps = n_bundles - 1;
        std::vector<uint32_t> run(counts.begin(), counts.begin() + n), next(n);
        std::vector<int> tops((size_t)2 * steps * tiles);
        std::vector<uint32_t> rows(steps);
        auto top_of = [](const int *t, size_t count) { int m = 0; for (size_t i = 0; i < count; i++) m = std::max(m, t[i]); return (uint32_t)m; };
        for (uint32_t k = 0; k < steps; k++) {
            const uint32_t *cb = counts.data() + (size_t)(k + 1) * n;
            merge_counts(run.data(), cb, n, max_items, next.data());
            const std::vector<int> ta = merge_tile_tops(run.data(), n), tb = merge_tile_tops(cb, n);
            std::copy(ta.begin(), ta.end(), tops.begin() + (size_t)2 * k * tiles);
            std::copy(tb.begin(), tb.end(), tops.begin() + (size_t)(2 * k + 1) * tiles);
            rows[k] = top_of(ta.data(), tiles) + top_of(tb.data(), tiles) + 1;
            if (top_of(tb.data(), tiles) > bundles[k + 1]->degree || (!k && top_of(ta.data(), tiles) > bundles[0]->degree))
                throw std::logic_error("merge: a bin count exceeds its BinBundle's degree");
            run.swap(next);
        }
        const std::vector<int> tfinal = merge_tile_tops(run.data(), n);
        const uint32_t degree = top_of(tfinal.data(), tiles);
        int *dtops = ws_as<int>(tops.size());
        HIP_CHECK(hipMemcpyAsync(dtops, tops.data(), tops.size() * sizeof(int), hipMemcpyHostToDevice, st_));
        // (rows[] adds the largest counts of two inputs, which need not be in the same slot: an early step can be the tallest)
        const uint32_t most_rows = *std::max_element(rows.begin(), rows.end());
        u64 *buf[2] = { ws((size_t)most_rows * n), steps > 1 ? ws((size_t)most_rows * n) : nullptr };
        merge_evs_.record(2, st_);
        const u64 *cur = poly[0];
        for (uint32_t k = 0; k < steps; k++) {
            u64 *out = buf[(steps - 1 - k) & 1];                       // the last step writes buf[0]
            launch_bins_merge(cur, dtops + (size_t)2 * k * tiles, poly[k + 1], dtops + (size_t)(2 * k + 1) * tiles, make_mod(hp_.t), out, n, rows[k], st_);
            cur = out;
        }
        merge_evs_.record(3, st_);
        b = new_bundle(bundles[0]->bundle_idx, cache_idx, degree);
        encode_bundle(*b, cur);                                        // rows above `degree` are 0: rows[] is a bound over tiles, degree over slots
        merge_evs_.record(4, st_);
        sync();
    });
    pack_bundle(*b);
    const int span[3][2] = { { 0, 1 }, { 2, 3 }, { 3, 4 } };
    for (int i = 0; i < 3; i++) merge_ms_[i] = merge_evs_.ms(span[i][0], span[i][1]);
    return b;
}

void Engine::merge_times(double *decode_ms, double *kernel_ms, double *encode_ms)
{
    Enter g(this);
    if (decode_ms) *decode_ms = merge_ms_[0];
    if (kernel_ms) *kernel_ms = merge_ms_[1];
    if (encode_ms) *encode_ms = merge_ms_[2];
}

Engine::CompactResult Engine::compact(uint32_t bundle_idx, const Bundle *const *bundles, uint32_t n_bundles)
{
    CompactResult res;
    const size_t n = hp_.n;
    {
        Enter g(this);
        TIER1_SLOTS();
        lookup_check("compact");
        if (bundle_idx >= psu_.bundle_idx_count) throw std::invalid_argument("bundle_idx out of range");
        check_one_index_in_cache_order(bundle_idx, bundles, n_bundles);
        std::vector<uint32_t> counts((size_t)n_bundles * n);
        if (n_bundles) lookup_impl(bundles, n_bundles, nullptr, nullptr, 0, counts.data(), nullptr);
        res.plan = plan_compaction(counts.data(), n_bundles, n, psu_.table_params.max_items_per_bin);
    }
    // the context's lock is taken per merge from here on, as by a caller who made these calls one by one; the given BinBundles are only read
    res.merged.resize(res.plan.degree.size());
    for (size_t g = 0; g < res.merged.size(); g++) {
        std::vector<const Bundle *> members;
        for (uint32_t b = 0; b < n_bundles; b++)
            if (res.plan.group[b] == g) members.push_back(bundles[b]);
        if (members.size() >= 2) res.merged[g] = merge_bundles(members.data(), (uint32_t)members.size(), members[0]->cache_idx);
    }
    return res;
}

// ---- N2 towards the reference: a resident BinBundle as BinBundle::save writes it (wire.h: build_bin_bundle; bin_rows.h)
void Engine::keep_coeff_rows(const Bundle &b, const u64 *coeff, DevBuf &keep)
{
    const size_t n = hp_.n;
    const size_t H = b.use_ps ? b.H : 0;
    keep.alloc((H + 1) * n * sizeof(u64));
    D2D(keep.u(), coeff, n);
    for (const BundleRun &r : layout_of(b.degree).runs)
        if (r.kind == COEFF_LIFTED)
            for (uint32_t i = 0; i < r.count; i++) D2D(keep.u() + (1 + r.first_slot + i) * n, coeff + (size_t)(r.d0 + i) * n, n);
}

static double host_ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

std::vector<uint8_t> Engine::export_saved(const Bundle &b, const u64 ntt_parms_id[4], uint32_t flags, int compr)
{
    Enter g(this);
    TIER1_SLOTS();
    lookup_check("export_saved");
    if (flags & ~(uint32_t)(SAVED_STRIPPED | SAVED_NO_CACHE)) throw std::invalid_argument("export_saved: unknown flag");
    const bool stripped = (flags & SAVED_STRIPPED) != 0, cache = !(flags & SAVED_NO_CACHE);
    if (stripped && !cache) throw std::invalid_argument("export_saved: a stripped BinBundle holds nothing but its cache, so STRIPPED and NO_CACHE together leave nothing to save");
    if (compr != sealio::COMPR_NONE && compr != sealio::COMPR_ZSTD) throw std::invalid_argument("export_saved: compr_mode is none (0) or zstd (2)");
    const size_t n = hp_.n;
    const uint32_t bins = psu_.bins_per_bundle, max_items = psu_.table_params.max_items_per_bin, degree = b.degree;
    // (unstripped, the same bound comes out of the bin counts below, with the bin's name)
    if (stripped && degree + 1 > max_items)
        throw std::invalid_argument("export_saved: the BinBundle has " + std::to_string(degree + 1) + " plaintexts, BinBundle::load accepts max_items_per_bin = " +
                                    std::to_string(max_items) + " at most");
    const BundleLayout y = layout_of(degree);
    for (double &m : export_ms_) m = 0;
    export_evs_.reserve(3);

    std::vector<u64> rows, row_off, bin_felts, bin_off;
    DevBuf keep;                                                       // a_0 and the a_{i h} in coefficient form mod t
    double copy_ms = 0;
    if (!stripped) {
        // what the tap takes from bundle_bins' decode while the columns are whole
        struct Tap : BinsTap {
            Engine *e; const Bundle *b; uint32_t bins, max_items; bool cache;
            std::vector<u64> *rows, *row_off; DevBuf *keep; double *copy_ms;
            void after_counts(const u64 *poly, const u64 *coeff, const uint32_t *dcounts, const uint32_t *counts) override
            {
                const size_t n = e->hp_.n;
                // a bin may hold max_items_per_bin - 1 items (receiver_db.cpp:388-389); build_bundle lets one more in, and its polynomial
                // of max_items_per_bin + 1 coefficients is what BinBundle::load's cache check refuses
                for (uint32_t s = 0; s < bins; s++)
                    if (counts[s] != LOOKUP_NONE && counts[s] >= max_items)
                        throw std::invalid_argument("bin " + std::to_string(s) + " holds " + std::to_string(counts[s]) + " items: a saved BinBundle has at most max_items_per_bin - 1 = " +
                                                    std::to_string(max_items - 1) + " per bin (BinBundle::load refuses the cache otherwise)");
                *row_off = rows_offsets(counts, bins, b->degree + 1);
                if (!cache) return;
                // BinBundle::load wants as many plaintexts as the longest matching polynomial has coefficients (bin_bundle.cpp:1356-1366): a
                // BinBundle uploaded with plaintexts above every bin's count has more
                uint32_t longest = 0;
                for (uint32_t s = 0; s < bins; s++) longest = std::max(longest, counts[s]);
                if (longest != b->degree)
                    throw std::invalid_argument("export_saved: the BinBundle has degree " + std::to_string(b->degree) + " but its longest bin holds " + std::to_string(longest) +
                                                " items: BinBundle::load refuses a cache whose plaintexts outnumber the longest matching polynomial's coefficients");
                const std::vector<int> tops = rows_tile_tops(counts, n, bins);
                const u64 total = row_off->back();
                u64 *doff = e->ws(row_off->size()), *dout = e->ws(total + 1);
                int *dtops = e->ws_as<int>(tops.size());
                HIP_CHECK(hipMemcpyAsync(doff, row_off->data(), row_off->size() * sizeof(u64), hipMemcpyHostToDevice, e->st_));
                HIP_CHECK(hipMemcpyAsync(dtops, tops.data(), tops.size() * sizeof(int), hipMemcpyHostToDevice, e->st_));
                e->export_evs_.record(0, e->st_);
                launch_bins_rows(poly, n, b->degree + 1, dcounts, doff, dtops, bins, dout, e->st_);
                e->export_evs_.record(1, e->st_);
                e->keep_coeff_rows(*b, coeff, *keep);
                e->sync();
                const auto t0 = std::chrono::steady_clock::now();
                rows->resize(total);
                if (total) HIP_CHECK(hipMemcpy(rows->data(), dout, total * sizeof(u64), hipMemcpyDeviceToHost));   // one contiguous copy
                *copy_ms = host_ms_since(t0);
                e->export_evs_.record(2, e->st_);
            }
        } tap;
        tap.e = this; tap.b = &b; tap.bins = bins; tap.max_items = max_items; tap.cache = cache;
        tap.rows = &rows; tap.row_off = &row_off; tap.keep = &keep; tap.copy_ms = &copy_ms;
        const uint32_t stride = std::max<uint32_t>(1, degree);
        std::vector<u64> roots(n * (size_t)stride);
        std::vector<uint32_t> counts(n);
        bins_impl(b, roots.data(), counts.data(), stride, BINS_FORM_AUTO, &tap);
        double tap_ms = 0;
        if (cache) { export_ms_[2] = export_evs_.ms(0, 1); tap_ms = export_evs_.ms(0, 2); }
        export_ms_[0] = bins_ms_[0];
        export_ms_[1] = std::max(0.0, bins_ms_[1] - tap_ms) + bins_ms_[2];
        bin_off.assign((size_t)bins + 1, 0);
        for (uint32_t s = 0; s < bins; s++) bin_off[s + 1] = bin_off[s] + counts[s];
        bin_felts.resize(bin_off[bins]);
        for (uint32_t s = 0; s < bins; s++) std::copy(roots.data() + (size_t)s * stride, roots.data() + (size_t)s * stride + counts[s], bin_felts.begin() + bin_off[s]);
    } else {
        // stripped: nothing but a_0 and the a_{i h} is decoded -- decode_bundle's steps up to the un-lift, on the H lifted slots alone
        const size_t H = b.use_ps ? b.H : 0;
        const int high = hp_.clamp_chain_idx(1);
        keep.alloc((H + 1) * n * sizeof(u64));
        D2D(keep.u(), b.a0.u(), n);
        if (H) {
            const size_t Lh = (size_t)high + 1, sb = b.packed ? b.lifted_slot_bytes : Lh * n * sizeof(u64);
            launch_limb0_rows(dlevel(high), (int)Lh, b.lifted.p(), sb, b.packed, keep.u() + n, n, H, st_);
            d_ntt(keep.u() + n, H, map_ct(), 1, true, data_primes_narrow_);
            launch_unlift(keep.u() + n, H * n, hp_.t, hp_.key_q[0], st_);
        }
        sync();
    }

    // the plaintexts, one degree at a time: the whole dense BinBundle is never on the host
    std::vector<std::vector<uint8_t>> blobs;
    double ser_ms = 0;
    if (cache) {
        const size_t Lpt = (size_t)b.pt_level + 1;
        blobs.resize((size_t)degree + 1);
        std::vector<u64> host(std::max(Lpt, (size_t)1) * n);
        DevBuf dense;
        if (b.packed && b.ntt_count) dense.alloc(Lpt * n * sizeof(u64));
        for (uint32_t d = 0; d <= degree; d++) {
            const BundleWhere w = y.where(d);
            const bool ntt = w.kind == COEFF_NTT;
            const size_t words = ntt ? Lpt * n : n;
            auto t0 = std::chrono::steady_clock::now();
            if (!ntt) HIP_CHECK(hipMemcpy(host.data(), keep.u() + (w.kind == COEFF_RAW ? 0 : 1 + w.slot) * n, words * sizeof(u64), hipMemcpyDeviceToHost));
            else if (b.packed) {
                launch_unpack_rows(dlevel(b.pt_level), (int)Lpt, static_cast<const char *>(b.ntt.p()) + w.slot * b.ntt_slot_bytes, b.ntt_slot_bytes, dense.u(), n, 1, st_);
                sync();
                HIP_CHECK(hipMemcpy(host.data(), dense.p(), words * sizeof(u64), hipMemcpyDeviceToHost));
            } else HIP_CHECK(hipMemcpy(host.data(), b.ntt.u() + w.slot * words, words * sizeof(u64), hipMemcpyDeviceToHost));
            copy_ms += host_ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            sealio::Plaintext pt;
            if (ntt) std::copy(ntt_parms_id, ntt_parms_id + 4, pt.parms_id);
            pt.coeff_count = words;
            pt.data.assign(host.begin(), host.begin() + words);
            blobs[d] = sealio::save_plaintext(pt, (uint8_t)compr);
            ser_ms += host_ms_since(t0);
        }
    }
    export_ms_[3] = copy_ms;
    export_ms_[4] = ser_ms;

    const auto t0 = std::chrono::steady_clock::now();
    wire::BinBundleParts parts;
    parts.bundle_idx = b.bundle_idx;
    parts.mod = hp_.t;
    parts.stripped = stripped;
    parts.has_cache = cache;
    parts.bin_felts = bin_felts.data(); parts.bin_off = bin_off.data(); parts.n_bins = stripped ? 0 : bins;
    parts.polyn_felts = rows.data(); parts.polyn_off = row_off.data(); parts.n_polyns = stripped || !cache ? 0 : bins;
    for (const auto &blob : blobs) parts.coeffs.push_back(wire::Span{ blob.data(), blob.size() });
    std::vector<uint8_t> out = wire::build_bin_bundle(parts);           // (refuses a buffer over the 32-bit limit before it allocates)
    export_ms_[5] = host_ms_since(t0);
    return out;
}

void Engine::export_times(double ms[6])
{
    Enter g(this);
    for (int i = 0; i < 6; i++) ms[i] = export_ms_[i];
}

// ---- N2: BinBundle image ------------------------------------------------------------------------------------
void Engine::algebraize_items(const unsigned char *items, size_t count, bool items_on_device, u64 *out, bool out_on_device)
{
    Enter g(this);
    if (!has_psu_) throw std::logic_error("context was created without PSUParams");
    if (!count) return;
    TIER1_SLOTS();
    const u32 felts = psu_.item_params.felts_per_item, bpf = psu_.item_bit_count_per_felt, bits = psu_.item_bit_count;
    WITH_ARENA({
        const unsigned char *src = items;
        if (!items_on_device) {
            unsigned char *d = ws_as<unsigned char>(count * 16);
            HIP_CHECK(hipMemcpyAsync(d, items, count * 16, hipMemcpyHostToDevice, st_));
            src = d;
        }
        u64 *dst = out_on_device ? out : ws(count * felts);
        { PROF(P_OTHER, 0); launch_algebraize(src, count, felts, bpf, bits, dst, st_); }
        if (!out_on_device) D2H(out, dst, count * felts);
        sync();
    });
}

namespace {
struct ImageHeader {                     // little-endian, 256 bytes
    char magic[8];                       // "APSUHEB2"
    uint64_t header_bytes, total_bytes;
    uint64_t n, t, K, q[8];
    uint32_t ps_low_degree, max_items_per_bin;
    uint32_t bundle_idx, cache_idx, degree, use_ps, H, r, pt_level, row_format;   // row_format: 0 dense 64-bit words, 1 bit-packed rows (was `reserved`)
    uint64_t ntt_count, ntt_bytes, lifted_bytes, a0_bytes;
    uint64_t checksum;                   // checksum64 over the payload
    unsigned char pad[256 - 8 - 16 - 88 - 8 - 32 - 32 - 8];
};
static_assert(sizeof(ImageHeader) == 256, "image header layout");
uint64_t fnv1a64(const unsigned char *p, size_t n, uint64_t h = 1469598103934665603ull)
{
    for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}
// Payload checksum: four interleaved FNV-1a-style lanes over 64-bit little-endian words, folded together with the tail bytes and
// the length at the end.  (Byte-serial FNV-1a, the "APSUHEB1" images of round 2, is one dependent multiply per byte: under
// 1 GB/s, minutes for a 75 GiB database on every load; this runs at memory speed.)
uint64_t checksum64(const unsigned char *p, size_t n)
{
    const uint64_t P = 1099511628211ull;
    uint64_t h[4] = { 1469598103934665603ull, 0x9e3779b97f4a7c15ull, 0xc2b2ae3d27d4eb4full, 0x165667b19e3779f9ull };
    size_t i = 0;
    for (; i + 32 <= n; i += 32) {
        uint64_t w[4];
        std::memcpy(w, p + i, 32);
        for (int k = 0; k < 4; k++) h[k] = (h[k] ^ w[k]) * P;
    }
    uint64_t r = fnv1a64(p + i, n - i);
    for (int k = 0; k < 4; k++) { r = (r ^ h[k]) * P; r ^= r >> 31; }
    return r ^ (uint64_t)n;
}
}

size_t Engine::bundle_image_size(const Bundle &b) const { return sizeof(ImageHeader) + b.ntt.bytes() + b.lifted.bytes() + b.a0.bytes(); }

size_t Engine::save_bundle(const Bundle &b, unsigned char *buf, size_t capacity)
{
    Enter g(this);
    if (!has_psu_) throw std::logic_error("context was created without PSUParams");
    const size_t total = bundle_image_size(b);
    if (capacity < total) throw std::invalid_argument("image buffer too small");
    sync();
    ImageHeader hd;
    std::memset(&hd, 0, sizeof(hd));
    std::memcpy(hd.magic, "APSUHEB2", 8);
    hd.header_bytes = sizeof(hd); hd.total_bytes = total;
    hd.n = hp_.n; hd.t = hp_.t; hd.K = hp_.K;
    for (int j = 0; j < hp_.K && j < 8; j++) hd.q[j] = hp_.key_q[j];
    hd.ps_low_degree = psu_.query_params.ps_low_degree; hd.max_items_per_bin = psu_.table_params.max_items_per_bin;
    hd.bundle_idx = b.bundle_idx; hd.cache_idx = b.cache_idx; hd.degree = b.degree; hd.use_ps = b.use_ps; hd.H = b.H; hd.r = b.r;
    hd.pt_level = (uint32_t)b.pt_level; hd.ntt_count = b.ntt_count; hd.row_format = b.packed ? 1 : 0;
    hd.ntt_bytes = b.ntt.bytes(); hd.lifted_bytes = b.lifted.bytes(); hd.a0_bytes = b.a0.bytes();
    unsigned char *p = buf + sizeof(hd);
    if (hd.ntt_bytes) HIP_CHECK(hipMemcpy(p, b.ntt.p(), hd.ntt_bytes, hipMemcpyDeviceToHost));
    p += hd.ntt_bytes;
    if (hd.lifted_bytes) HIP_CHECK(hipMemcpy(p, b.lifted.p(), hd.lifted_bytes, hipMemcpyDeviceToHost));
    p += hd.lifted_bytes;
    HIP_CHECK(hipMemcpy(p, b.a0.p(), hd.a0_bytes, hipMemcpyDeviceToHost));
    hd.checksum = checksum64(buf + sizeof(hd), total - sizeof(hd));
    std::memcpy(buf, &hd, sizeof(hd));
    return total;
}

std::unique_ptr<Bundle> Engine::load_bundle(const unsigned char *buf, size_t size)
{
    Enter g(this);
    if (!has_psu_) throw std::logic_error("context was created without PSUParams");
    ImageHeader hd;
    if (size < sizeof(hd)) throw std::invalid_argument("BinBundle image is truncated");
    std::memcpy(&hd, buf, sizeof(hd));
    if (std::memcmp(hd.magic, "APSUHEB2", 8) != 0 || hd.header_bytes != sizeof(hd)) throw std::invalid_argument("not a BinBundle image");
    if (hd.total_bytes != size || hd.total_bytes != sizeof(hd) + hd.ntt_bytes + hd.lifted_bytes + hd.a0_bytes)
        throw std::invalid_argument("BinBundle image size mismatch");
    bool same = hd.n == hp_.n && hd.t == hp_.t && hd.K == (uint64_t)hp_.K && hd.ps_low_degree == psu_.query_params.ps_low_degree &&
                hd.max_items_per_bin == psu_.table_params.max_items_per_bin;
    for (int j = 0; same && j < hp_.K && j < 8; j++) same = hd.q[j] == hp_.key_q[j];
    if (!same) throw std::invalid_argument("BinBundle image was built for different parameters");
    if (checksum64(buf + sizeof(hd), size - sizeof(hd)) != hd.checksum) throw std::invalid_argument("BinBundle image is corrupt (checksum)");
    BundleLayout y;                                               // the header must say what the layout says
    auto b = new_bundle(hd.bundle_idx, hd.cache_idx, hd.degree, &y);
    const size_t n = hp_.n;
    if (hd.row_format > 1 || (hd.row_format == 1 && !hp_.using_keyswitching)) throw std::invalid_argument("BinBundle image header is inconsistent");
    const bool img_packed = hd.row_format == 1;
    const size_t ntt_slot = slot_bytes(b->pt_level, img_packed), lift_slot = slot_bytes(hp_.clamp_chain_idx(1), img_packed);
    const size_t want_ntt = y.ntt_count ? y.ntt_count * ntt_slot + (img_packed ? 16 : 0) : 0;
    const size_t want_lift = y.lifted_count ? y.lifted_count * lift_slot + (img_packed ? 16 : 0) : 0;
    if (y.H != hd.H || y.r != hd.r || (uint32_t)y.use_ps != hd.use_ps || (uint32_t)y.pt_level != hd.pt_level || y.ntt_count != hd.ntt_count ||
        hd.ntt_bytes != want_ntt || hd.a0_bytes != n * sizeof(u64) || hd.lifted_bytes != want_lift || hd.bundle_idx >= psu_.bundle_idx_count)
        throw std::invalid_argument("BinBundle image header is inconsistent");
    const unsigned char *p = buf + sizeof(hd);
    b->ntt.alloc(hd.ntt_bytes); b->lifted.alloc(hd.lifted_bytes); b->a0.alloc(hd.a0_bytes);
    if (hd.ntt_bytes) HIP_CHECK(hipMemcpy(b->ntt.p(), p, hd.ntt_bytes, hipMemcpyHostToDevice));
    p += hd.ntt_bytes;
    if (hd.lifted_bytes) HIP_CHECK(hipMemcpy(b->lifted.p(), p, hd.lifted_bytes, hipMemcpyHostToDevice));
    p += hd.lifted_bytes;
    HIP_CHECK(hipMemcpy(b->a0.p(), p, hd.a0_bytes, hipMemcpyHostToDevice));
    b->packed = img_packed;
    if (img_packed) { b->ntt_slot_bytes = ntt_slot; b->lifted_slot_bytes = lift_slot; }
    // an image of the other row format is converted to this context's (APSU_HE_PACKED_ROWS)
    if (packed_rows_ && !b->packed) pack_bundle(*b);
    else if (!packed_rows_ && b->packed) unpack_bundle(*b);
    return b;
}

size_t Engine::download_coeff(const Bundle &b, uint32_t d, u64 *out, size_t capacity, int *kind)
{
    Enter g(this);
    sync();
    const size_t n = hp_.n;
    if (d > b.degree) throw std::invalid_argument("degree out of range");
    const BundleWhere w = layout_of(b.degree).where(d);
    if (w.kind == COEFF_LIFTED && !b.use_ps) throw std::invalid_argument("coefficient is not stored for this bundle");
    const int k = w.kind, lvl = k == COEFF_NTT ? b.pt_level : hp_.clamp_chain_idx(1);
    const DevBuf &buf = k == COEFF_RAW ? b.a0 : k == COEFF_NTT ? b.ntt : b.lifted;
    const size_t words = k == COEFF_RAW ? n : (size_t)(lvl + 1) * n;
    if (capacity < words) throw std::invalid_argument("output buffer too small");
    if (b.packed && k != COEFF_RAW) {                            // one bit-packed slot -> dense words
        const size_t sb = k == COEFF_NTT ? b.ntt_slot_bytes : b.lifted_slot_bytes;
        DevBuf tmp(words * sizeof(u64));
        launch_unpack_rows(dlevel(lvl), lvl + 1, static_cast<const char *>(buf.p()) + w.slot * sb, sb, tmp.u(), n, 1, st_);
        sync();
        HIP_CHECK(hipMemcpy(out, tmp.p(), words * sizeof(u64), hipMemcpyDeviceToHost));
    } else HIP_CHECK(hipMemcpy(out, buf.u() + w.slot * words, words * sizeof(u64), hipMemcpyDeviceToHost));
    if (kind) *kind = k;
    return words;
}

// ---- what a BinBundle answers in plaintext (bin_eval.h): decode, k_bin_counts, k_bins_eval, one BinBundle after the other through the
// workspace as the lookup runs them.  Queues only: inside the caller's WITH_ARENA, which syncs.  xs / masks: per BinBundle a device
// pointer to n slot values (masks, or an entry of it, may be null); out [n_bundles][n], is_bin [n_bundles][n] or null, bad: one zeroed
// word that a value >= t raises -- all device memory.
void Engine::eval_plain_queue(const Bundle *const *bundles, uint32_t n_bundles, const u64 *const *xs, const u64 *const *masks, u64 *out,
                              unsigned char *is_bin, u32 *bad)
{
    const size_t n = hp_.n;
    eval_evs_.reserve((size_t)4 * n_bundles);
    uint32_t *dcounts = ws_as<uint32_t>(n);
    const size_t mark = arena_off_;
    for (uint32_t i = 0; i < n_bundles; i++) {
        const Bundle &b = *bundles[i];
        arena_off_ = mark;                                             // one BinBundle after the other through the same workspace (stream order)
        eval_evs_.record(4 * i, st_);
        u64 *poly = ws((size_t)(b.degree + 1) * n);                    // [d][slot] slot values of the batched polynomial
        decode_bundle(b, poly);
        eval_evs_.record(4 * i + 1, st_);
        launch_bin_counts(poly, n, b.degree + 1, dcounts, st_);
        eval_evs_.record(4 * i + 2, st_);
        launch_bins_eval(poly, n, b.degree + 1, dcounts, xs[i], masks ? masks[i] : nullptr, make_mod(hp_.t), out + (size_t)i * n,
                         is_bin ? is_bin + (size_t)i * n : nullptr, bad, st_);
        eval_evs_.record(4 * i + 3, st_);
    }
}

// after the caller's sync
void Engine::eval_plain_collect(uint32_t n_bundles)
{
    eval_ms_[0] = eval_ms_[1] = eval_ms_[2] = 0;
    for (uint32_t i = 0; i < n_bundles; i++)
        for (int k = 0; k < 3; k++) eval_ms_[k] += eval_evs_.ms(4 * i + k, 4 * i + k + 1);
}

static void check_slot_values(const u64 *v, size_t rows, size_t n, u64 t, const char *what)
{
    for (size_t i = 0; i < rows * n; i++)
        if (v[i] >= t)
            throw std::invalid_argument(std::string(what) + " " + std::to_string(v[i]) + " (row " + std::to_string(i / n) + ", slot " + std::to_string(i % n) +
                                        ") is not reduced modulo plain_modulus");
}

void Engine::bundles_eval_plain(const Bundle *const *bundles, uint32_t n_bundles, const u64 *x, bool x_on_device, const u64 *masks, bool masks_on_device,
                                u64 *out, bool out_on_device, unsigned char *is_bin)
{
    Enter g(this);
    TIER1_SLOTS();
    lookup_check("eval_plain");
    if (!n_bundles) return;
    const size_t n = hp_.n, words = (size_t)n_bundles * n;
    if (!x_on_device) check_slot_values(x, n_bundles, n, hp_.t, "slot value");
    if (masks && !masks_on_device) check_slot_values(masks, n_bundles, n, hp_.t, "mask value");
    u32 bad_host = 0;
    WITH_ARENA({
        const u64 *dx = x, *dm = masks;
        if (!x_on_device) {
            u64 *staged = ws(words);
            HIP_CHECK(hipMemcpyAsync(staged, x, words * sizeof(u64), hipMemcpyHostToDevice, st_));
            dx = staged;
        }
        if (masks && !masks_on_device) {
            u64 *staged = ws(words);
            HIP_CHECK(hipMemcpyAsync(staged, masks, words * sizeof(u64), hipMemcpyHostToDevice, st_));
            dm = staged;
        }
        u64 *dout = out_on_device ? out : ws(words);
        unsigned char *dbin = !is_bin ? nullptr : out_on_device ? is_bin : ws_as<unsigned char>(words);
        u32 *bad = ws_as<u32>(1, 1);
        HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(u64), st_));
        std::vector<const u64 *> xs(n_bundles), ms(n_bundles);
        for (uint32_t i = 0; i < n_bundles; i++) { xs[i] = dx + (size_t)i * n; ms[i] = dm ? dm + (size_t)i * n : nullptr; }
        eval_plain_queue(bundles, n_bundles, xs.data(), ms.data(), dout, dbin, bad);
        if (!out_on_device) {
            HIP_CHECK(hipMemcpyAsync(out, dout, words * sizeof(u64), hipMemcpyDeviceToHost, st_));
            if (is_bin) HIP_CHECK(hipMemcpyAsync(is_bin, dbin, words, hipMemcpyDeviceToHost, st_));
        }
        HIP_CHECK(hipMemcpyAsync(&bad_host, bad, sizeof(u32), hipMemcpyDeviceToHost, st_));
        sync();
    });
    eval_plain_collect(n_bundles);
    if (bad_host) throw std::invalid_argument("a slot or mask value on the device is not reduced modulo plain_modulus");
}

void Engine::eval_plain_times(double *decode_ms, double *counts_ms, double *kernel_ms)
{
    Enter g(this);
    if (decode_ms) *decode_ms = eval_ms_[0];
    if (counts_ms) *counts_ms = eval_ms_[1];
    if (kernel_ms) *kernel_ms = eval_ms_[2];
}

// ---- the self-test (include/apsu_he.h: apsu_he_db_self_test): the querier's and the receiver's calls strung together on device buffers
// of this call, then the plaintext answer and the comparison.  The context's lock is taken per step, as by a caller who made these calls
// one by one; the BinBundles are only read.
SelfTestReport Engine::self_test(const Bundle *const *bundles, uint32_t count, const u64 seed[8], const u64 *x_host, const uint32_t *query_indices,
                                 uint32_t n_query, const uint32_t *mask_positions)
{
    SelfTestReport rep = self_test_empty();
    std::vector<uint32_t> idx;
    {
        Enter g(this);
        lookup_check("self_test");
        if (!hp_.using_keyswitching) throw std::invalid_argument("parameters do not support key switching: the reference creates no relinearisation keys");
        if (query_indices) idx.assign(query_indices, query_indices + n_query);
        else {
            for (uint32_t i = 0; i < count; i++) idx.push_back(bundles[i]->bundle_idx);
            std::sort(idx.begin(), idx.end());
            idx.erase(std::unique(idx.begin(), idx.end()), idx.end());
        }
        for (size_t k = 0; k < idx.size(); k++)
            if (idx[k] >= psu_.bundle_idx_count || (k && idx[k] <= idx[k - 1])) throw std::invalid_argument("bundle indices are ascending, distinct and in range");
        for (uint32_t i = 0; i < count; i++) {
            if (!std::binary_search(idx.begin(), idx.end(), bundles[i]->bundle_idx)) throw std::invalid_argument("a BinBundle's bundle index is not among the query's");
            if (mask_positions && mask_positions[i] >= SELF_TEST_MAX_OBJECTS) throw std::invalid_argument("too many BinBundles for one self-test");
        }
        if (count >= SELF_TEST_MAX_OBJECTS) throw std::invalid_argument("too many BinBundles for one self-test");
    }
    if (!count) return rep;
    const size_t n = hp_.n;
    const int K = hp_.K, L = hp_.first_chain_idx + 1, n_idx = (int)idx.size();
    const size_t S = psu_.query_params.query_powers.size();
    if (x_host) check_slot_values(x_host, idx.size(), n, hp_.t, "slot value");
    Blake2xbSeed sd;
    for (int i = 0; i < 8; i++) sd.w[i] = seed[i];
    auto pos = [&](uint32_t i) { return mask_positions ? mask_positions[i] : i; };

    DevBuf xs, mvals, menc, sk, cts, res, got, want;                   // allocated with the context's device current
    std::unique_ptr<RelinKeys> rk;
    std::unique_ptr<Powers> pw;
    // the key material of the call is overwritten before its buffers are released, whichever way the call ends: the secret key, the
    // relinearisation keys, and the workspace through which keygen and the key generation passed them
    auto wipe = [&] {
        try {
            Enter g(this);
            if (sk.bytes()) HIP_CHECK(hipMemsetAsync(sk.p(), 0, sk.bytes(), st_));
            if (rk && rk->data.bytes()) HIP_CHECK(hipMemsetAsync(rk->data.p(), 0, rk->data.bytes(), st_));
            if (arena_.bytes()) HIP_CHECK(hipMemsetAsync(arena_.p(), 0, arena_.bytes(), st_));
            sync();
        } catch (...) { }
    };
    try {
        {
            Enter g(this);
            self_evs_.reserve(4);
            xs.alloc(idx.size() * n * sizeof(u64)); mvals.alloc((size_t)count * n * sizeof(u64)); menc.alloc((size_t)count * n * sizeof(u64));
            sk.alloc((size_t)K * n * sizeof(u64)); cts.alloc(idx.size() * S * 2 * L * n * sizeof(u64)); res.alloc((size_t)count * 2 * n * sizeof(u64));
            got.alloc((size_t)count * n * sizeof(u64)); want.alloc((size_t)count * n * sizeof(u64));
            if (x_host) HIP_CHECK(hipMemcpyAsync(xs.p(), x_host, xs.bytes(), hipMemcpyHostToDevice, st_));
            else launch_fill_blake2xb(xs.u(), idx.size() * n, sd, SELF_TEST_X_FIRST, hp_.t, st_);
            // the masks' slot values, position by position: the draws apsu_he_mask_generate_blake2xb encodes below
            for (uint32_t i = 0; i < count; i++) launch_fill_blake2xb(mvals.u() + (size_t)i * n, n, sd, SELF_TEST_MASK_FIRST + (u64)pos(i) * n, hp_.t, st_);
            self_evs_.record(0, st_);
        }
        keygen(seed, sk.u(), true);
        relin_keygen(sk.u(), seed, nullptr, nullptr, &rk, true);
        std::vector<u64> ct_seeds(idx.size() * S * 8);
        query_create(sk.u(), seed, idx.data(), n_idx, xs.u(), true, cts.u(), ct_seeds.data(), true);
        std::vector<const u64 *> src(idx.size() * S);
        for (size_t c = 0; c < src.size(); c++) src[c] = cts.u() + c * 2 * L * n;
        pw = compute_powers(idx.data(), n_idx, src.data(), true, rk.get());
        for (uint32_t i = 0; i < count;) {                             // runs of consecutive positions continue one stream
            uint32_t j = i + 1;
            while (j < count && pos(j) == pos(j - 1) + 1) j++;
            mask_generate_blake2xb(seed, SELF_TEST_MASK_FIRST + (u64)pos(i) * n, j - i, menc.u() + (size_t)i * n, nullptr, nullptr);
            i = j;
        }
        std::vector<const u64 *> mptr(count), xptr(count), vptr(count);
        for (uint32_t i = 0; i < count; i++) {
            mptr[i] = menc.u() + (size_t)i * n;
            vptr[i] = mvals.u() + (size_t)i * n;
            xptr[i] = xs.u() + (size_t)(std::lower_bound(idx.begin(), idx.end(), bundles[i]->bundle_idx) - idx.begin()) * n;
        }
        eval_bundles(bundles, (int)count, *pw, rk.get(), mptr.data(), true, res.u(), true);
        std::vector<int> budget(count);
        decrypt_decode(sk.u(), res.u(), true, count, nullptr, nullptr, budget.data(), true, got.u());
        u64 status[2] = { 0, EVAL_NO_MISMATCH };
        u32 bad_host = 0;
        {
            Enter g(this);
            TIER1_SLOTS();
            WITH_ARENA({
                self_evs_.record(1, st_);
                u64 *dstatus = ws(2);
                u32 *bad = ws_as<u32>(1, 1);
                const u64 init[2] = { 0, EVAL_NO_MISMATCH };
                HIP_CHECK(hipMemcpyAsync(dstatus, init, sizeof(init), hipMemcpyHostToDevice, st_));
                HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(u64), st_));
                eval_plain_queue(bundles, count, xptr.data(), vptr.data(), want.u(), nullptr, bad);
                self_evs_.record(2, st_);
                launch_eval_compare(got.u(), want.u(), n, count, dstatus, st_);
                self_evs_.record(3, st_);
                HIP_CHECK(hipMemcpyAsync(status, dstatus, sizeof(status), hipMemcpyDeviceToHost, st_));
                HIP_CHECK(hipMemcpyAsync(&bad_host, bad, sizeof(u32), hipMemcpyDeviceToHost, st_));
                sync();
            });
            eval_plain_collect(count);
            if (bad_host) throw std::logic_error("self_test: a drawn value is not reduced modulo plain_modulus");
            rep.bundles = count;
            rep.slots = (u64)count * n;
            rep.mismatches = status[0];
            if (status[1] != EVAL_NO_MISMATCH) {
                rep.first_bundle = (int32_t)(status[1] >> 32);
                rep.first_slot = (uint32_t)status[1];
                const size_t at = (size_t)rep.first_bundle * n + rep.first_slot;
                HIP_CHECK(hipMemcpy(&rep.first_got, got.u() + at, sizeof(u64), hipMemcpyDeviceToHost));
                HIP_CHECK(hipMemcpy(&rep.first_expected, want.u() + at, sizeof(u64), hipMemcpyDeviceToHost));
            }
            for (uint32_t i = 0; i < count; i++)
                if (rep.min_budget_bundle < 0 || budget[i] < rep.min_budget_bits) { rep.min_budget_bits = budget[i]; rep.min_budget_bundle = (int32_t)i; }
            rep.he_ms = self_evs_.ms(0, 1);
            rep.plain_ms = self_evs_.ms(1, 3);
            self_ms_[0] = eval_ms_[0]; self_ms_[1] = eval_ms_[1]; self_ms_[2] = eval_ms_[2];
            self_ms_[3] = self_evs_.ms(2, 3);
            self_ms_[4] = rep.he_ms;
        }
    } catch (...) {
        wipe();
        if (pw) recycle_powers(std::move(pw));
        throw;
    }
    wipe();
    recycle_powers(std::move(pw));
    return rep;
}

void Engine::self_test_times(double ms[5])
{
    Enter g(this);
    for (int i = 0; i < 5; i++) ms[i] = self_ms_[i];
}

} // namespace apsu_he
