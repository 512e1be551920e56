// See engine.h.  What makes, stores and converts a BinBundle: uploaded, generated, built from bins, encoded and decoded, copied between
// contexts, saved and loaded as an image.  The calls on a resident database are in engine_db.cpp.
// Where each coefficient of a BinBundle is stored is decided in bundle_layout.h alone; this file shares with the query path
// (engine.cpp) the arena, the streams and the transform launcher (engine_impl.h).
#include "engine_impl.h"

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
        pack_rows_grid_check(b.ntt_count, b.pt_level + 1);
        launch_pack_rows(dlevel(b.pt_level), b.pt_level + 1, b.ntt.u(), pk.p(), b.ntt_slot_bytes, n, b.ntt_count, st_);
        sync();
        b.ntt = std::move(pk);
    }
    if (H) {
        DevBuf pk;
        pk.alloc(H * b.lifted_slot_bytes + 16);
        HIP_CHECK(hipMemsetAsync(static_cast<char *>(pk.p()) + H * b.lifted_slot_bytes, 0, 16, st_));
        pack_rows_grid_check(H, high + 1);
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
        pack_rows_grid_check(b.ntt_count, b.pt_level + 1);
        launch_unpack_rows(dlevel(b.pt_level), b.pt_level + 1, b.ntt.p(), b.ntt_slot_bytes, dn.u(), n, b.ntt_count, st_);
        sync();
        b.ntt = std::move(dn);
    }
    const size_t H = b.use_ps ? b.H : 0;
    if (H && b.lifted.bytes()) {
        DevBuf dn;
        dn.alloc(H * (size_t)(high + 1) * n * sizeof(u64));
        pack_rows_grid_check(H, high + 1);
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
    lookup_check(nullptr, NEED_PSU);
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
    lookup_check(nullptr, NEED_PSU);
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
    lookup_check(nullptr, NEED_BATCHING);
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
    for (uint32_t s = 0; s < bins; s++) check_reduced(roots + (size_t)s * stride, counts[s], hp_.t, field_element);
    auto b = new_bundle(bundle_idx, cache_idx, degree);
    WITH_ARENA({
        u64 *droots = ws((size_t)bins * stride + 1);
        uint32_t *dcounts = ws_as<uint32_t>(bins, 1);
        if (bins) {
            H2D(droots, roots, (size_t)bins * stride);
            HIP_CHECK(hipMemcpyAsync(dcounts, counts, bins * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
        }
        build_from_roots(*b, droots, dcounts, bins, stride);
        sync();
    });
    pack_bundle(*b);
    return b;
}

void Engine::build_from_roots(Bundle &b, const u64 *droots, const uint32_t *dcounts, uint32_t bins, uint32_t stride)
{
    const size_t n = hp_.n;
    u64 *poly = ws((size_t)(b.degree + 1) * n);                    // [d][slot] slot values of the batched polynomial
    launch_polyn_with_roots(droots, dcounts, bins, stride, b.degree, make_mod(hp_.t), poly, n, st_);
    encode_bundle(b, poly);
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
    const size_t n = hp_.n;
    u64 *raw = ws((size_t)(degree + 1) * n);
    decode_coeff(b, raw);
    if (coeff) D2D(coeff, raw, (size_t)(degree + 1) * n);
    d_ntt(raw, degree + 1, map_ct() + hp_.plain_id(), 1, false, false);
    launch_gather_slots(raw, reinterpret_cast<const uint32_t *>(d_slot_map_.p()), poly, n, (int)degree + 1, st_);
}

void Engine::decode_coeff(const Bundle &b, u64 *raw)
{
    const uint32_t degree = b.degree;
    const size_t n = hp_.n, Lpt = b.pt_level + 1;
    const int high = hp_.clamp_chain_idx(1);
    const size_t Lh = high + 1;
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
}

std::unique_ptr<Bundle> Engine::clone_bundle(const Bundle &src, int src_device)
{
    Enter g(this);
    lookup_check(nullptr, NEED_PSU);
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

// ---- N2: BinBundle image ------------------------------------------------------------------------------------
void Engine::algebraize_items(const unsigned char *items, size_t count, bool items_on_device, u64 *out, bool out_on_device)
{
    Enter g(this);
    lookup_check(nullptr, NEED_PSU);
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
    lookup_check(nullptr, NEED_PSU);
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
    lookup_check(nullptr, NEED_PSU);
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

} // namespace apsu_he
