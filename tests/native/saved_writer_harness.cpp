// Stand-alone driver of the saved-database writers (apsu_amd/csrc/wire.h: build_bin_bundle, build_receiver_db_header) against the
// readers next to them, meant to be built with -fsanitize=address,undefined (tests/test_saved_db_writer_cpu.py).  Every buffer handed
// to a reader is an exact-size heap copy, so a read past its end is seen.  Prints "ok" and returns 0, or says what differed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "wire.h"

using namespace apsu_he;

namespace {

[[noreturn]] void fail(const std::string &what)
{
    std::fprintf(stderr, "FAILED: %s\n", what.c_str());
    std::exit(1);
}
#define EXPECT(cond) do { if (!(cond)) fail(std::string(#cond) + " (line " + std::to_string(__LINE__) + ")"); } while (0)

struct Ragged {
    std::vector<uint64_t> felts, off{ 0 };
    void row(const std::vector<uint64_t> &r) { felts.insert(felts.end(), r.begin(), r.end()); off.push_back(felts.size()); }
    size_t rows() const { return off.size() - 1; }
    std::vector<uint64_t> at(size_t i) const { return std::vector<uint64_t>(felts.begin() + off[i], felts.begin() + off[i + 1]); }
};

std::unique_ptr<uint8_t[]> exact_copy(const uint8_t *p, size_t n)
{
    std::unique_ptr<uint8_t[]> c(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(c.get(), p, n);
    return c;
}

wire::BinBundleParts parts_of(uint32_t idx, uint64_t mod, const Ragged &bins, const Ragged &polyns, const std::vector<std::vector<uint8_t>> &blobs, bool stripped,
                              bool cache)
{
    wire::BinBundleParts p;
    p.bundle_idx = idx; p.mod = mod; p.stripped = stripped; p.has_cache = cache;
    p.bin_felts = bins.felts.data(); p.bin_off = bins.off.data(); p.n_bins = bins.rows();
    p.polyn_felts = polyns.felts.data(); p.polyn_off = polyns.off.data(); p.n_polyns = polyns.rows();
    for (const auto &b : blobs) p.coeffs.push_back(wire::Span{ b.data(), b.size() });
    return p;
}

void check_round_trip(uint32_t idx, uint64_t mod, const Ragged &bins, const Ragged &polyns, const std::vector<std::vector<uint8_t>> &blobs, bool stripped,
                      bool cache, std::vector<uint8_t> *keep = nullptr)
{
    const wire::BinBundleParts p = parts_of(idx, mod, bins, polyns, blobs, stripped, cache);
    const std::vector<uint8_t> buf = wire::build_bin_bundle(p);
    EXPECT(buf.size() == wire::bin_bundle_bytes(p));
    EXPECT(buf.size() % 4 == 0);
    const auto copy = exact_copy(buf.data(), buf.size());
    const wire::SavedBinBundle sb = wire::parse_bin_bundle(copy.get(), buf.size(), true);
    EXPECT(sb.consumed == buf.size() && sb.bundle_idx == idx && sb.mod == mod && sb.stripped == stripped && sb.has_cache == cache);
    EXPECT(sb.has_label_bins && sb.label_bins == 0);
    EXPECT(sb.item_bins.size() == (stripped ? 0 : bins.rows()));
    for (size_t i = 0; i < sb.item_bins.size(); i++) EXPECT(sb.item_bins[i] == bins.at(i));
    if (cache) {
        EXPECT(sb.has_felt_interp && sb.felt_interp == 0 && sb.has_batched_interp && sb.batched_interp == 0);
        EXPECT(sb.matching_polyns.size() == (stripped ? 0 : polyns.rows()));
        for (size_t i = 0; i < sb.matching_polyns.size(); i++) EXPECT(sb.matching_polyns[i] == polyns.at(i));
        EXPECT(sb.batched_coeffs.size() == blobs.size());
        for (size_t d = 0; d < blobs.size(); d++)
            EXPECT(sb.batched_coeffs[d].n == blobs[d].size() && (blobs[d].empty() || !std::memcmp(sb.batched_coeffs[d].p, blobs[d].data(), blobs[d].size())));
    } else EXPECT(sb.batched_coeffs.empty() && sb.matching_polyns.empty());
    if (keep) *keep = buf;
}

}  // namespace

int main()
{
    const uint64_t mod = 65537;
    Ragged bins, polyns, none;
    const std::vector<std::vector<uint64_t>> item_rows = { { 5, 7, 11 }, {}, { ((uint64_t)1 << 40) + 3 }, { 1, 2, 3, 4, 5, 6, 7, 8 }, {} };
    for (const auto &r : item_rows) {
        bins.row(r);
        std::vector<uint64_t> poly(r.size() + 1, 3);                  // (any values: the writer does not look at them)
        poly.back() = 1;
        polyns.row(poly);
    }
    std::vector<std::vector<uint8_t>> blobs;
    for (int d = 0; d < 9; d++) blobs.push_back(std::vector<uint8_t>((size_t)(10 + 7 * d), (uint8_t)(d + 1)));
    blobs.push_back({});                                              // an empty byte vector is a byte vector

    std::vector<uint8_t> full, stripped, nocache;
    check_round_trip(3, mod, bins, polyns, blobs, false, true, &full);
    check_round_trip(0, mod, bins, polyns, blobs, true, true, &stripped);
    check_round_trip(1, mod, bins, none, {}, false, false, &nocache);
    check_round_trip(2, ((uint64_t)1 << 59) + 1, none, none, { blobs[0] }, false, true);

    // three buffers one behind the other, walked by `consumed`
    std::vector<uint8_t> cat = full;
    cat.insert(cat.end(), stripped.begin(), stripped.end());
    cat.insert(cat.end(), nocache.begin(), nocache.end());
    {
        const auto copy = exact_copy(cat.data(), cat.size());
        size_t at = 0;
        const uint32_t want_idx[3] = { 3, 0, 1 };
        for (int i = 0; i < 3; i++) {
            const wire::SavedBinBundle sb = wire::parse_bin_bundle(copy.get() + at, cat.size() - at);
            EXPECT(sb.bundle_idx == want_idx[i]);
            at += sb.consumed;
        }
        EXPECT(at == cat.size());
    }

    // every truncated prefix of one written buffer is refused, none is followed out of bounds
    size_t refused = 0;
    for (size_t len = 0; len < full.size(); len++) {
        const auto copy = exact_copy(full.data(), len);
        try { (void)wire::parse_bin_bundle(len ? copy.get() : nullptr, len, true); fail("a truncated BinBundle of " + std::to_string(len) + " bytes was accepted"); }
        catch (const std::runtime_error &) { refused++; }
    }
    EXPECT(refused == full.size());

    // refusals of the writer itself
    try { (void)wire::build_bin_bundle(parts_of(0, mod, bins, polyns, blobs, true, false)); fail("stripped without a cache was written"); }
    catch (const std::invalid_argument &) {}
    try { wire::check_saved_size((uint64_t)1 << 31, "x"); fail("2^31 bytes accepted"); } catch (const std::invalid_argument &) {}
    wire::check_saved_size(((uint64_t)1 << 31) - 1, "x");

    // the header
    const std::vector<uint8_t> params(77, 0x5a), key = [] { std::vector<uint8_t> k(32); for (int i = 0; i < 32; i++) k[(size_t)i] = (uint8_t)(i * 3); return k; }();
    std::vector<uint64_t> hashed;
    for (uint64_t i = 0; i < 7; i++) { hashed.push_back(11 * i + 1); hashed.push_back(((uint64_t)1 << 63) + i); }
    for (int variant = 0; variant < 3; variant++) {
        wire::ReceiverDbHeaderParts h;
        h.params = wire::Span{ params.data(), params.size() };
        h.oprf_key = wire::Span{ key.data(), key.size() };
        h.hashed_items = variant == 2 ? nullptr : hashed.data();
        h.n_hashed_items = variant == 2 ? 0 : 7;
        h.item_count = 123; h.bin_bundle_count = variant == 1 ? 0 : 4; h.nonce_byte_count = 16;
        h.compressed = variant == 1; h.stripped = variant == 2;
        const std::vector<uint8_t> buf = wire::build_receiver_db_header(h);
        const auto copy = exact_copy(buf.data(), buf.size());
        const wire::ReceiverDbHeader r = wire::parse_receiver_db_header(copy.get(), buf.size());
        EXPECT(r.consumed == buf.size() && r.item_count == 123 && r.bin_bundle_count == h.bin_bundle_count && r.nonce_byte_count == 16 && r.label_byte_count == 0);
        EXPECT(r.compressed == h.compressed && r.stripped == h.stripped && r.hashed_item_count == h.n_hashed_items);
        EXPECT(r.params.n == params.size() && !std::memcmp(r.params.p, params.data(), params.size()));
        EXPECT(r.oprf_key.n == 32 && !std::memcmp(r.oprf_key.p, key.data(), 32));
        EXPECT(r.hashed_items.n == 16 * h.n_hashed_items && (!h.n_hashed_items || !std::memcmp(r.hashed_items.p, hashed.data(), r.hashed_items.n)));
        for (size_t len = 0; len < buf.size(); len++) {
            const auto cut = exact_copy(buf.data(), len);
            try { (void)wire::parse_receiver_db_header(len ? cut.get() : nullptr, len); fail("a truncated header was accepted"); }
            catch (const std::runtime_error &) {}
        }
    }
    std::printf("round trips, %zu truncated prefixes refused\nok\n", refused);
    return 0;
}
