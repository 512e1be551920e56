// Device-resident query-evaluation engine: the MI355X replacement for the seal::Evaluator calls
// made by apsu::receiver::Receiver::ComputePowers (receiver/apsu/receiver_osn.cpp:395-488) and
// BatchedPlaintextPolyn::eval / eval_patstock (receiver/apsu/bin_bundle.cpp:106-174,192-360).
//
// Tier 1 = one method per Evaluator call (host buffers in SEAL's [poly][limb][coeff] order),
// used for parity testing and incremental adoption.  Tier 2 = the fused, HBM-resident path:
// BinBundle plaintexts are uploaded once, ComputePowers runs level-synchronously over the
// PowersDag for all bundle indices at once, and every BinBundle of a query is evaluated in a
// few batched launches.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "device.h"
#include "params.h"
#include "db_place.h"
#include "db_compact.h"
#include "bulk_place.h"
#include "powers_dag.h"
#include "powers_sched.h"
#include "bundle_layout.h"

namespace apsu_he {

struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };

class DevBuf {                       // RAII device allocation
public:
    DevBuf() = default;
    explicit DevBuf(size_t bytes) { alloc(bytes); }
    ~DevBuf() { release(); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { release(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; } return *this; }
    void alloc(size_t bytes);
    void release();
    u64 *u() const { return static_cast<u64 *>(p_); }
    void *p() const { return p_; }
    size_t bytes() const { return bytes_; }
private:
    void *p_ = nullptr;
    size_t bytes_ = 0;
};

struct RelinKeys {                   // [decomp K-1][2][K][n], NTT form (SEAL KSwitchKeys data, index 0)
    DevBuf data;
};

// One uploaded BinBundle cache = the batched matching polynomial of BatchedPlaintextPolyn
// (bin_bundle.h:52-134): coefficient d for all bins, stored per the ctor's rule (bin_bundle.cpp:385-420), which bundle_layout.h
// decides: degree .. ntt_count below are copied from its BundleLayout (Engine::new_bundle), the evaluation reads them.
struct Bundle {
    uint32_t bundle_idx = 0, cache_idx = 0;
    uint32_t degree = 0;             // batched_coeffs.size() - 1
    bool use_ps = false;             // (ps_low_degree > 1) && (ps_low_degree < degree)  receiver_osn.cpp:520-522
    uint32_t H = 0, r = 0;           // degree / h, degree % h          (bin_bundle.cpp:225-227)
    int pt_level = 0;                // chain index of the NTT-form plaintexts
    size_t ntt_count = 0;            // NTT-form coefficients, packed in ascending degree order
    DevBuf ntt;                      // [ntt_count][pt_level+1][n]
    DevBuf lifted;                   // PS only: NTT(lift(a_{i*h})) at the high level, i = 1..H : [H][Lh][n]
    DevBuf a0;                       // constant coefficient, n words mod t
    // Row format of `ntt` and `lifted` (round 4).  false: dense 64-bit words as above.  true: every plaintext is a slot of
    // ntt_slot_bytes / lifted_slot_bytes bytes whose limb rows are bit-packed (DevLevel::mac_bits: 7 bytes per coefficient of a
    // 56-bit prime, 6.25 of a 50-bit one); both buffers carry 16 spare bytes behind the last slot (k_mac reads 16-byte windows).
    bool packed = false;
    size_t ntt_slot_bytes = 0, lifted_slot_bytes = 0;
    size_t db_bytes() const { return ntt.bytes() + lifted.bytes() + a0.bytes(); }
};

// Output of ComputePowers for a set of bundle indices (CiphertextPowers, receiver_osn.h:41).
struct Powers {
    int nb = 0;                                  // bundle indices held
    std::vector<uint32_t> bundle_indices;
    int low_level = 0, high_level = 0;
    uint32_t n_low = 0, n_high = 0;              // PS: l low powers, H high powers; no PS: all in `low`
    uint32_t polys = 2;                          // polynomials stored per power (the "2" of the layouts below).  More than 2 only without
                                                 // key switching: products are never relinearised, every power is stored zero-padded to
                                                 // the longest one's size rounded up to even (Engine::power_size gives the real sizes)
    DevBuf low;                                  // [idx][power-1][2][Ll][n]   NTT form
    DevBuf high;                                 // [idx][i-1][2][Lh][n]       coefficient form (power i*h)
    DevBuf hext;                                 // [idx][i-1][2][Eh][n]       extended + NTT form of the same
    // high/hext are produced on the engine's second stream when the PowersDag splits (see Engine::compute_powers);
    // consumers on the main stream wait for this event first.  Null / never recorded = already ordered.
    hipEvent_t high_ready = nullptr;
    bool high_async = false;
    bool low_async = false;                      // pipelined queries (Engine::compute_powers): the low powers come from the second stream too
    // recorded on the main stream behind the last evaluation that read these powers: when the buffer comes back from the pool,
    // the second stream may start writing its high half as soon as THAT evaluation is over -- it does not have to wait for whatever
    // else the main stream has queued since (Engine::compute_powers, inputs_ready_)
    mutable hipEvent_t last_use = nullptr;
    mutable bool last_use_set = false;
    // sequence number of the ComputePowers call that filled this buffer: the word a source coefficient outside [0, q) is reported in
    // (Engine::check_sources) carries it, so the report attaches to THIS query's evaluation / download
    uint32_t seq = 0;
    ~Powers() { if (high_ready) (void)hipEventDestroy(high_ready); if (last_use) (void)hipEventDestroy(last_use); }
    Powers() = default;
    Powers(const Powers &) = delete;
    Powers &operator=(const Powers &) = delete;
    int slot_of(uint32_t bundle_idx) const;
};

struct PsBatch;
struct EvalPlan;                     // eval_plan.h (engine_eval.cpp)

// time stamps of a resident-database call on the engine's stream: events created before the call's first stamp (outside the timed
// spans), elapsed times read after the call's sync
struct EventStamps {
    std::vector<hipEvent_t> ev;
    void reserve(size_t count);
    void record(size_t i, hipStream_t st);
    double ms(size_t from, size_t to) const;
    void release();
};

// apply_entries' host step: what a lookup found (counts [n_bundles][n], present [n_bundles][n_rem + n_ins] with the removals first, both
// in cache order) -> place_entries (db_place.h).  Engine::apply_entries and MultiEngine::apply_entries share it.
PlaceResult place_from_lookup(uint32_t n_bundles, size_t n, uint32_t bins, uint32_t F, uint32_t max_items, u64 t, const uint32_t *counts,
                              const unsigned char *present, const u64 *ins_felts, const uint32_t *ins_start, size_t n_ins, const u64 *rem_felts,
                              const uint32_t *rem_start, size_t n_rem);

class Engine {
public:
    Engine(const HeParams &hp, const PSUParams *psu, int device);
    ~Engine();

    const HeParams &he() const { return hp_; }
    const PSUParams *psu() const { return has_psu_ ? &psu_ : nullptr; }
    const PowersDag &dag() const { return dag_; }
    hipStream_t stream() const { return st_; }
    void sync();

    // ---------------- tier 1 (host pointers; each call is H2D, kernels, D2H)
    void transform_to_ntt(u64 *ct, int polys, int chain_idx);
    void transform_from_ntt(u64 *ct, int polys, int chain_idx);
    void multiply_plain_ntt(const u64 *ct, const u64 *pt_ntt, u64 *out, int polys, int chain_idx);
    void multiply_plain(const u64 *ct, const u64 *pt, size_t pt_coeffs, u64 *out, int polys, int chain_idx);
    void transform_plain_to_ntt(const u64 *pt, size_t pt_coeffs, u64 *out, int chain_idx);
    void add(u64 *acc, const u64 *x, int polys, int chain_idx);
    void add_plain(u64 *ct, const u64 *pt, size_t pt_coeffs, int chain_idx);
    void multiply(const u64 *a, const u64 *b, u64 *out3, int chain_idx);
    // Evaluator::multiply for operands of any size (nothing relinearised in between): out has size_a + size_b - 1 polynomials
    void multiply_sized(const u64 *a, int size_a, const u64 *b, int size_b, u64 *out, int chain_idx);
    void relinearize(u64 *ct3, const RelinKeys &rk, int chain_idx);
    void mod_switch_to_next(u64 *ct, int polys, int chain_idx);
    void clear_irrelevant_bits(u64 *ct, int polys);

    // ---------------- tier 2 (device resident)
    std::unique_ptr<RelinKeys> upload_relin_keys(const u64 *rk_host);
    std::unique_ptr<Bundle> upload_bundle(uint32_t bundle_idx, uint32_t cache_idx, uint32_t n_coeffs,
                                          const u64 *const *coeff_ptrs, const unsigned char *is_ntt);
    // Synthetic-DB helper for benchmarks: fills a bundle of the given degree with uniformly random
    // plaintext coefficients generated and transformed on the GPU (no host data).
    std::unique_ptr<Bundle> random_bundle(uint32_t bundle_idx, uint32_t cache_idx, uint32_t degree, u64 seed);
    // N1: BinBundle::regen_polyns + regen_plaintexts + BatchedPlaintextPolyn ctor on the GPU
    // (bin_bundle.cpp:366-430,934-1026): roots[bin * stride + r], r < counts[bin], are the field elements of a bin.
    std::unique_ptr<Bundle> build_bundle(uint32_t bundle_idx, uint32_t cache_idx, const u64 *roots, const uint32_t *counts,
                                         uint32_t bins, uint32_t stride);
    // N1, the update (ReceiverDB::insert_or_assign / remove -> BinBundle::multi_insert / try_multi_remove -> regen_cache,
    // receiver_db.cpp:330-433): a new BinBundle = `old` with bin s divided by (x - r) for its rem_counts[s] removal roots, then
    // multiplied by (x - r) for its ins_counts[s] insertion roots.  Needs no roots of `old`: its stored coefficients are decoded back
    // to the bins' polynomials mod t.  `old` is only read.  Semantics: include/apsu_he.h (apsu_he_bundle_update).
    std::unique_ptr<Bundle> update_bundle(const Bundle &old, const u64 *ins_roots, const uint32_t *ins_counts, uint32_t ins_stride,
                                          const u64 *rem_roots, const uint32_t *rem_counts, uint32_t rem_stride, uint32_t bins);
    // N1, find and place (include/apsu_he.h: apsu_he_bundle_bin_counts, apsu_he_bundles_lookup, apsu_he_db_apply_entries): what the
    // reference keeps on the host next to a BinBundle (item_bins_, the cuckoo filters, hashed_items_) is asked of the resident
    // polynomials instead.  counts: n words (host), LOOKUP_NONE where the slot is not a bin.
    void bin_counts(const Bundle &b, uint32_t *counts);
    // felts[count][felts_per_item], start[count]; present / room: [n_bundles][count] (host), either may be null
    void lookup_bundles(const Bundle *const *bundles, uint32_t n_bundles, const u64 *felts, const uint32_t *start, size_t count,
                        unsigned char *present, uint32_t *room);
    // the same call for a caller that places entries itself (MultiEngine: the BinBundles of one bundle index lie on several contexts):
    // counts [n_bundles][n] and present [n_bundles][count] (host) of these BinBundles, in the given order.  count == 0: counts alone.
    // n_bundles == 0: only the context's own refusals (what apply_entries and compact check before any GPU work).
    void lookup_counts(const char *what, const Bundle *const *bundles, uint32_t n_bundles, const u64 *felts, const uint32_t *start, size_t count,
                       uint32_t *counts, unsigned char *present);
    // a BinBundle of ANOTHER context with the same parameters (on src_device) as a BinBundle of this one: its three arrays go device to
    // device on this context's stream (hipMemcpyPeerAsync), no host image.  `src` is only read; the copy is complete on return.
    std::unique_ptr<Bundle> clone_bundle(const Bundle &src, int src_device);
    // The resident-database calls' clock: one entry per operation, written by that operation alone.  op_times: the first `count` spans
    // in ms of the context's last such call (0 before the first):
    //   OP_LOOKUP     (bin_counts / lookup_bundles / apply_entries / compact, summed over the BinBundles) decode_bundle, the kernels behind it
    //   OP_BINS       (bundle_bins) decode and counts, the root search, multiplicities and copy-back
    //   OP_MERGE      (merge_bundles) the decodes and counts, the product kernels, the re-encode
    //   OP_EVAL_PLAIN (bundles_eval_plain, summed over the BinBundles) decode_bundle, k_bin_counts, k_bins_eval
    //   OP_SELF_TEST  (self_test) decode, k_bin_counts, k_bins_eval (summed over the BinBundles), the comparison, the homomorphic part
    //   OP_EXPORT     (export_saved) decode and counts, the root search and multiplicities, k_bins_rows (device, by events); the copies
    //                 to the host, the plaintexts' serialisation, the buffer's assembly (host clock)
    //   OP_SPLIT      (split_bundle) decode and counts, the root search and multiplicities, k_roots_split, the parts' builds
    //   OP_BUILD      (build_from_entries, summed over the bundle indices and BinBundles) the entries' copies, k_entries_scatter, the builds
    //   OP_BUCKET     (items_bucket_device) k_cuckoo_locations, the grouping (keys, passes, offsets and order), k_entries_gather
    enum Op { OP_LOOKUP = 0, OP_BINS, OP_MERGE, OP_EVAL_PLAIN, OP_SELF_TEST, OP_EXPORT, OP_SPLIT, OP_BUILD, OP_BUCKET, OP_COUNT };
    static constexpr int OP_SPANS = 6;
    void op_times(Op op, double *ms, int count);
    struct ApplyResult {
        PlaceResult place;                                 // per-entry status and target, per-BinBundle state (db_place.h)
        std::vector<std::unique_ptr<Bundle>> replaced;     // [n_bundles]: the new BinBundle where state == PLACE_REPLACED, else null
        std::vector<std::unique_ptr<Bundle>> appended;     // [place.n_new]
    };
    // lookup -> place_entries -> update_bundle per changed BinBundle -> build_bundle per appended one, for the BinBundles of one bundle
    // index given in cache order.  The given BinBundles are only read.
    ApplyResult apply_entries(uint32_t bundle_idx, const Bundle *const *bundles, uint32_t n_bundles, const u64 *ins_felts, const uint32_t *ins_start,
                              size_t n_ins, const u64 *rem_felts, const uint32_t *rem_start, size_t n_rem);
    // N1, a whole database from its entries (include/apsu_he.h: apsu_he_db_build_from_entries; bulk_place.h): ReceiverDB::set_data on an
    // empty database.  entries [offsets[table_size]][16]: the post-OPRF items in items_bucket's order, host or device; offsets
    // [table_size + 1] (host).  Per bundle index with entries: its contiguous entry range is copied once, its kstart uploaded; per
    // BinBundle k in cache order new_bundle(b, k, degree), k_entries_scatter into root lists from the arena, build_from_roots -- no
    // entry touches the host.  cache_idx = k.  Out: bundle index by bundle index, in cache order within each; a bundle index without
    // entries gets no BinBundle.  want (may be null: all): one byte per BinBundle of the plan in that order, 0 = not built here, a null
    // pointer in its place (MultiEngine builds each on its device).  NO entry-level dedupe: two equal entries of one location put a
    // double root into their bins.  All or nothing.
    BulkPlan entries_plan(const u64 *offsets) const;
    std::vector<std::unique_ptr<Bundle>> build_from_entries(const unsigned char *entries, bool on_device, const u64 *offsets, const unsigned char *want = nullptr);
    // measurement hook: workgroups per location of k_entries_scatter in build_from_entries; 0 (the default) = scatter_blocks' choice
    void set_scatter_blocks(uint32_t blocks) { std::lock_guard<std::mutex> g(mu_); scatter_blocks_ = blocks; }
    // N1, compaction (include/apsu_he.h: apsu_he_bundles_merge, apsu_he_db_compact): the union of two bins is the product of their
    // polynomials, so n >= 2 BinBundles of one bundle index become ONE new BinBundle without anybody's roots: decode each, per-slot
    // products pairwise (k_bins_merge, bin_merge.h), the tail of the build.  The given BinBundles are only read.
    std::unique_ptr<Bundle> merge_bundles(const Bundle *const *bundles, uint32_t n_bundles, uint32_t cache_idx);
    // N1, reading the bins back (include/apsu_he.h: apsu_he_bundle_bins; bin_roots.h): the roots of every bin's polynomial, found as the
    // zeros of (t - 1) / n forward transforms mod t of the bin's scaled coefficients.  counts: n words (host), LOOKUP_NONE where the slot
    // is not a bin; roots (host, may be null): bin s at roots[s * stride], ascending, a value of multiplicity m written m times.
    // form: BINS_FORM_AUTO, or one of the two paths by name (the debug call of the tests).  `b` is only read.
    enum { BINS_FORM_AUTO = 0, BINS_FORM_KERNEL = 1, BINS_FORM_COMPOSED = 2 };
    void bundle_bins(const Bundle &b, u64 *roots, uint32_t *counts, uint32_t stride, int form = BINS_FORM_AUTO);
    // N1, splitting (include/apsu_he.h: apsu_he_bundle_split; bin_split.h): the inverse of merge_bundles.  bundle_bins' decode, counts and
    // root search, then k_roots_split sorts and cuts every bin's list on the device and the tail of the build makes each part from
    // the device-resident lists: no root reaches the host, which knows every part's counts and degree from the counts alone.  Part p
    // holds positions [split_cut(c, k, p), split_cut(c, k, p + 1)) of every bin's sorted list, keeps b's bundle_idx and takes
    // cache_idx[p] (null: b's own and the numbers behind it).  `b` is only read.
    std::vector<std::unique_ptr<Bundle>> split_bundle(const Bundle &b, uint32_t k, const uint32_t *cache_idx);
    // N1, moving (apsu_he_bundle_adopt, apsu_he_db_rebase; db_rebase.h), called on the DESTINATION: a BinBundle of `src`, a context on
    // the same device whose parameters are rebase_compatible with this one's, becomes a BinBundle of this context with the given
    // cache_idx -- the coefficient half of src's decode, then this context's finish_bundle.  No slot transform, no roots.  The two
    // contexts' locks are taken one after the other, never together.  `b` is only read.
    std::unique_ptr<Bundle> adopt_bundle(Engine &src, const Bundle &b, uint32_t cache_idx);
    struct RebaseResult { std::vector<std::unique_ptr<Bundle>> bundles; std::vector<uint32_t> origin; };
    // bin_counts per BinBundle in src -> rebase_plan -> adopt_bundle, or split_bundle in src and adopt_bundle of each part (the parts
    // are released).  All or nothing.  origin[i]: the position in `bundles` that output i came from.
    RebaseResult rebase_from(Engine &src, const Bundle *const *bundles, uint32_t n_bundles);
    // What a BinBundle answers in plaintext (include/apsu_he.h: apsu_he_bundles_eval_plain; bin_eval.h): out[b][s] = P_s(x[b][s]) + masks[b][s]
    // mod t for the polynomial P_s that BinBundle b holds in slot s -- the value a querier decrypts there.  x, masks (may be null), out:
    // [n_bundles][n] slot values, host or device as flagged; is_bin (may be null): [n_bundles][n] bytes on out's side, 0 where the slot
    // holds the zero polynomial.  The BinBundles are only read.
    void bundles_eval_plain(const Bundle *const *bundles, uint32_t n_bundles, const u64 *x, bool x_on_device, const u64 *masks, bool masks_on_device,
                            u64 *out, bool out_on_device, unsigned char *is_bin);
    // The self-test (include/apsu_he.h: apsu_he_db_self_test): keygen, relin_keygen, query_create, compute_powers, the masks, eval_bundles and
    // decrypt_decode on device buffers of the call, held slot for slot against bundles_eval_plain of the same values.  x_host (may be
    // null: drawn from the seed): [distinct bundle indices, ascending][n].  For a handle that tests one database in parts (MultiEngine):
    // query_indices = the bundle indices of the whole (ascending; x_host then follows them) and mask_positions[i] = the position of
    // BinBundle i in the whole, so every part draws what one context would draw.  Positions in the report are positions in `bundles`.
    SelfTestReport self_test(const Bundle *const *bundles, uint32_t count, const u64 seed[8], const u64 *x_host, const uint32_t *query_indices = nullptr,
                             uint32_t n_query = 0, const uint32_t *mask_positions = nullptr);
    // N2 towards the reference (include/apsu_he.h: apsu_he_bundle_export_saved): the BinBundle as BinBundle::save writes it
    // (wire.h: build_bin_bundle), read by the reference's BinBundle::load and by apsu_he_db_upload_saved_bundle.  ntt_parms_id: SEAL's
    // parms_id of chain level b.pt_level (the engine does not hash parameters; the SEAL context of the C ABI does).  One decode serves
    // the bins (bundle_bins), the bins' polynomials (k_bins_rows, bin_rows.h) and the coefficient-form plaintexts; the NTT-form ones
    // are the stored rows, unpacked one degree at a time.  compr: sealio::COMPR_NONE or COMPR_ZSTD.  `b` is only read.
    enum { SAVED_STRIPPED = 1, SAVED_NO_CACHE = 2 };
    std::vector<uint8_t> export_saved(const Bundle &b, const u64 ntt_parms_id[4], uint32_t flags, int compr);
    struct CompactResult {
        CompactPlan plan;                                  // group per BinBundle, degree per group (db_compact.h)
        std::vector<std::unique_ptr<Bundle>> merged;       // [groups]: the new BinBundle of a group of two or more, else null
    };
    // bin_counts per BinBundle -> plan_compaction -> merge_bundles per group of two or more, for the BinBundles of one bundle index
    // given in cache order
    CompactResult compact(uint32_t bundle_idx, const Bundle *const *bundles, uint32_t n_bundles);
    // N1, one step earlier: algebraize_item (common/apsu/util/db_encoding.cpp:209-256,360-366) for `count` hashed items of 16 bytes:
    // out[count][felts_per_item], felt j = bits [j*b, (j+1)*b) of the item's first item_bit_count bits, b = bit_count(t) - 1
    void algebraize_items(const unsigned char *items, size_t count, bool items_on_device, u64 *out, bool out_on_device);
    // N1, cuckoo hashing for both parties (include/apsu_he.h: apsu_he_item_locations ... apsu_he_query_values; cuckoo.h, engine_cuckoo.cpp).
    // item_locations: locs[count][hash_func_count] of `count` items of 16 bytes (k_cuckoo_locations).  items_bucket: the same
    // locations, then the stable grouping by location on the host (cuckoo_bucket): offsets[table_size + 1], order[count * hash_func_count]
    // (host).  cuckoo_table: the querier's table by the engine's rule (k_cuckoo_insert): table_idx[table_size], item_loc[count], rounds
    // (host; rounds may be null); an item without a slot after max_rounds: std::runtime_error naming the lowest one and the fill rate.
    // query_values: table_items [table_size][16], the table after the caller's OPRF -> values[bundle_idx_count][n] as query_create reads them.
    void item_locations(const unsigned char *items, size_t count, bool items_on_device, uint32_t *locs, bool locs_on_device);
    void items_bucket(const unsigned char *items, size_t count, bool items_on_device, u64 *offsets, uint32_t *order, u64 *total);
    void cuckoo_table(const unsigned char *items, size_t count, bool items_on_device, u64 max_rounds, uint32_t *table_idx, uint32_t *item_loc, u64 *rounds);
    void query_values(const unsigned char *table_items, bool on_device, u64 *values, bool values_on_device);
    // items_bucket with the grouping and the gather on the device (include/apsu_he.h: apsu_he_items_bucket_device; bucket_plan.h,
    // kernels_bucket.hip): the same offsets (host) and order, and entries[k] = items[order[k]] as build_from_entries reads them.  order
    // and entries may be null, and host or device memory as flagged; only offsets must visit the host.
    void items_bucket_device(const unsigned char *items, size_t count, bool items_on_device, u64 *offsets, uint32_t *order, bool order_on_device,
                             unsigned char *entries, bool entries_on_device, u64 *total);
    // test hook: the grouping alone on caller-given locations locs[count][H] (host) in tiles of `tile` keys (0: BUCKET_TILE_DEFAULT), any
    // context; offsets [T + 1] and order (count * H words of room, host).  A location >= T: std::invalid_argument, nothing written.
    void debug_bucket_locs(const uint32_t *locs, size_t count, uint32_t H, uint32_t T, uint32_t tile, u64 *offsets, uint32_t *order, u64 *total);
    // test hook: k_cuckoo_insert alone on caller-given items and locations locs[count][H] (host), any context.  form: where the table
    // lives -- the engine's choice, LDS (std::logic_error where table_size slots do not fit), or device memory
    enum { CUCKOO_FORM_AUTO = 0, CUCKOO_FORM_LDS = 1, CUCKOO_FORM_GLOBAL = 2 };
    // test hook: k_cuckoo_locations alone with a caller-given function count and table size (host pointers), any context
    void debug_item_locations(const unsigned char *items, size_t count, uint32_t H, uint32_t T, uint32_t *locs);
    void debug_cuckoo_insert(const unsigned char *items, const uint32_t *locs, size_t count, uint32_t H, uint32_t T, u64 max_rounds, int form,
                             uint32_t *table_idx, uint32_t *item_loc, u64 *rounds);
    // N2: engine-native image of a BinBundle cache (raw limb arrays), replacing the flatbuffers +
    // SEAL-serialised blobs of ReceiverDB::save/Load (receiver_db.cpp:1182-1429) for the GPU-resident DB.
    size_t bundle_image_size(const Bundle &b) const;
    size_t save_bundle(const Bundle &b, unsigned char *buf, size_t capacity);
    std::unique_ptr<Bundle> load_bundle(const unsigned char *buf, size_t size);
    // N4: mask generation + block packing (receiver_osn.cpp:53-73,217-284) and the querier's
    // decrypt + decode + packing (result_package.cpp:175-213 ; sender_osn.cpp:675-700)
    void mask_generate(u64 seed, uint32_t count, u64 *masks_dev, u64 *values_host, u64 *blocks_host);
    // the same with the reference's generator: SEAL's Blake2xb PRNG under `seed`, starting at its first_value-th 32-bit output
    void mask_generate_blake2xb(const u64 seed[8], u64 first_value, uint32_t count, u64 *masks_dev, u64 *values_host, u64 *blocks_host);
    // budget_bits (may be null): SEAL's invariant noise budget of every result
    // sk_on_device: the key is device memory of this context (the self-test's, which never leaves the device) and is taken as it is, here
    // and in the three calls below; values_dev (may be null): the slot values once more, [count][n] on the device
    void decrypt_decode(const u64 *sk_ntt_host, const u64 *cts, bool on_device, uint32_t count, u64 *values_host, u64 *blocks_host,
                        int *budget_bits = nullptr, bool sk_on_device = false, u64 *values_dev = nullptr);
    // N5, the querier's side (query_side.h): Sender::reset_keys and create_query's HE half (sender/apsu/sender_osn.cpp:215-229,426-484)
    void keygen(const u64 seed[8], u64 *sk_ntt_host, bool sk_on_device = false);            // [K][n]
    // ksk_host [K-1][2][K][n], seeds_host [K-1][8] and resident may each be null
    void relin_keygen(const u64 *sk_ntt_host, const u64 seed[8], u64 *ksk_host, u64 *seeds_host, std::unique_ptr<RelinKeys> *resident,
                      bool sk_on_device = false);
    // cts_dev: [nb * S][2][L][n] device words; seeds_host: [nb * S][8]
    void query_create(const u64 *sk_ntt_host, const u64 seed[8], const uint32_t *bundle_indices, int nb, const u64 *values, bool values_on_device,
                      u64 *cts_dev, u64 *seeds_host, bool sk_on_device = false);
    // N3 on the device: c1 of `count` seeded objects at chain_idx (-1 / K - 1: the key level) = util::sample_poly_uniform under
    // SEAL's Blake2xb generator seeded with seeds[i][8], written to the DEVICE buffers dst[i] ([L][n] words each)
    void seed_expand(int chain_idx, int count, const u64 *seeds, u64 *const *dst);
    // test hook: stored form of coefficient d.  kind: 0 = raw mod t (d = 0), 1 = NTT form at pt_level,
    // 2 = pre-lifted + NTT at the high level (coefficient-form a_{i*h}); returns words written
    size_t download_coeff(const Bundle &b, uint32_t d, u64 *out, size_t capacity, int *kind);
    // src[b * n_sources + s]: source power s (ascending power order) of bundle index bundle_indices[b],
    // size-2 coefficient-form ct at the first data level.  on_device: pointers are device pointers.
    std::unique_ptr<Powers> compute_powers(const uint32_t *bundle_indices, int nb, const u64 *const *src, bool on_device,
                                           const RelinKeys *rk);
    // masks[i]: n words mod t (host, or device if on_device).  out: count * 2n words (host or device).
    // out_rows (optional, implies device-accessible destinations): result i goes to out_rows[i] (2n words) instead of
    // out + i * 2n -- rows of another device's buffer (peer access) or of page-locked host memory are written in place.
    void eval_bundles(const Bundle *const *bundles, int count, const Powers &pw, const RelinKeys *rk,
                      const u64 *const *masks, bool masks_on_device, u64 *out, bool out_on_device, u64 *const *out_rows = nullptr);

    // Parameter sets with one coefficient prime have no key switching: the reference then never relinearises
    // (receiver_osn.cpp:416,430-432 ; bin_bundle.cpp:308-310), so powers and results have more than two polynomials.
    // power_size: polynomials of a target power after ComputePowers; result_size: of one BinBundle's result;
    // result_polys: the largest result_size over all degrees = polynomials per row of eval_bundles' output (2 with key switching).
    // The numbers are powers_sched.h's (power_sizes, result_size_for, result_polys; CT_SIZE_MAX), made at creation.
    uint32_t power_size(uint32_t power) const;
    uint32_t result_size(const Bundle &b) const;
    uint32_t result_polys() const { return result_polys_; }

    // introspection for tests
    size_t workspace_bytes() const { return arena_.bytes(); }
    // Host-side events that cost a query time without showing up in any kernel: host waits taken inside the engine,
    // job-table uploads (cache misses) and hits, workspace-arena growths, powers-buffer allocations, wraps of the pinned
    // staging area.  Steady state = only hits move.  (apsu_he_debug_counters)
    enum Counter { C_HOST_SYNC = 0, C_JOB_UPLOAD, C_JOB_HIT, C_ARENA_GROW, C_POWERS_ALLOC, C_STAGE_WRAP, C_JOB_REALLOC, C_PIPELINED, C_COUNT };
    void counters_read(uint64_t *out, int capacity) const { for (int i = 0; i < capacity && i < C_COUNT; i++) out[i] = counters_[i]; }

    // ---------------- per-kernel timing with HIP events on the engine's stream (bench.py roofline)
    enum ProfKind { P_NTT_FWD = 0, P_NTT_INV, P_MAC, P_BEHZ_EXT, P_TENSOR, P_BEHZ_FINISH, P_KEYSWITCH, P_MODSWITCH, P_OTHER, P_NTT_FUSED, P_COUNT };
    struct ProfStats { double ms[P_COUNT]; uint64_t launches[P_COUNT]; uint64_t units[P_COUNT]; };
    void profile_enable(int mode);      // 0 off, 1 every kernel class, 2 NTT launches only (cheapest)
    void profile_read(ProfStats *out, bool reset);
    // ---------------- phase timers under the reference's STOPWATCH names (receiver_osn.cpp:167,403,504): device time from HIP
    // events on the engine's streams.  RunQuery = start of a compute_powers call .. end of the last eval_bundles call before the
    // next compute_powers; ComputePowers ends when BOTH streams of a two-stream walk have finished.
    enum Phase { PH_RUN_QUERY = 0, PH_COMPUTE_POWERS, PH_PROCESS_BIN_BUNDLE_CACHE, PH_COUNT };
    struct PhaseSummary { uint64_t count = 0; double sum_ms = 0, min_ms = 0, max_ms = 0; };      // cli/common_utils.cpp:54-76 prints these
    static const char *phase_name(int phase);
    void phase_enable(bool on);
    void phase_read(PhaseSummary *out, bool reset);            // out[PH_COUNT]; waits for the recorded work
    // two-stream ComputePowers: -1 = default policy (on for one or two bundle indices), 0 = off, 1 = on
    void set_two_stream(int mode) { std::lock_guard<std::mutex> g(mu_); two_stream_mode_ = mode < 0 ? -1 : (mode ? 1 : 0); }
    // device-resident evaluation results without the closing stream synchronisation (see apsu_he_set_async_results)
    void set_async_results(bool on) { std::lock_guard<std::mutex> g(mu_); async_results_ = on; }
    // apsu_he_set_query_overlap.  0: off (the second stream waits for everything the main stream has queued).  1: the caller's inputs are
    // complete at call time -- the second stream waits only for the last reader of the powers buffer it reuses, and a ComputePowers
    // that finds an evaluation still running takes the pipelined walk.  2: as 1 without the pipelined walk.  3: as 1 with the
    // pipelined walk taken whether or not the device is busy (tests: the walk's event chain is then exercised deterministically).
    void set_query_overlap(int mode)
    {
        std::lock_guard<std::mutex> g(mu_);
        inputs_ready_ = mode != 0;
        pipe_cp_ = mode == 1 || mode == 3;
        force_pipe_ = mode == 3;
    }
    // tier 1 on device-resident operands: the per-method calls take device pointers and return with their work queued on the
    // engine's stream (no host round trip per Evaluator call); see apsu_he_set_tier1_on_device
    void set_tier1_on_device(bool on) { std::lock_guard<std::mutex> g(mu_); tier1_device_ = on; }
    void wait();                                                  // locked sync() + check_sources()
    void drain();                                                 // locked sync() alone: never throws for a query's data (buffer growth in callers)
    // Has any ComputePowers whose work is complete found a source coefficient outside [0, q) that no call has reported yet?  Clears it.
    // Never throws: for callers that must finish their own protocol first (MultiEngine::eval_all, in front of a collective).
    bool take_bad_source();
    // test hook: copy one computed power to the host (serialised with the other calls on this context)
    void download_power(const Powers &pw, uint32_t bundle_idx, uint32_t power, u64 *out, size_t capacity_words, int *chain_idx,
                        int *is_ntt);
    int device() const { return device_; }
    // test hook (engine_steps.cpp; include/apsu_he.h: apsu_he_debug_run_step): ONE launch_* call of device.h on host arrays in that
    // launcher's documented layout, with this context's own constant blocks.  Step ids, flags and the argument block mirror the C ABI's.
    // Refuses (std::invalid_argument, nothing launched) whatever the launcher's input contract does not admit.
    enum Step { STEP_LEVEL_INFO = 0, STEP_BEHZ_EXT, STEP_DROP_BEHZ_EXT, STEP_TENSOR, STEP_TENSOR_CONV, STEP_TENSOR_SUM, STEP_BEHZ_FINISH,
                STEP_BEHZ_FINISH_SUM, STEP_KS_INNER, STEP_KS_MODDOWN, STEP_MODSWITCH, STEP_MODSWITCH_JOBS, STEP_I0_FINISH, STEP_EVAL_EPILOGUE,
                STEP_ADD_MANY, STEP_SUM_JOBS, STEP_ADD_PLAIN, STEP_DYADIC_PLAIN, STEP_LIFT,
                // the resident-database kernels (engine_db_steps.cpp): the mod-t launchers of device.h, same argument block
                STEP_POLYN_WITH_ROOTS, STEP_BINS_UPDATE, STEP_BIN_COUNTS, STEP_POLY_DEGREE, STEP_BINS_LOOKUP, STEP_BINS_MERGE, STEP_BINS_ROWS,
                STEP_BINS_EVAL, STEP_EVAL_COMPARE, STEP_ROOTS, STEP_UNLIFT,
                // the transforms (engine_ntt_steps.cpp): the launchers of launch_ntt.h with a caller-given limb-to-modulus map
                STEP_NTT_INFO, STEP_NTT, STEP_NTT_GATHER, STEP_INTT_TENSOR,
                // behind the existing ids, which stay: k_roots_split (engine_db_steps.cpp)
                STEP_ROOTS_SPLIT,
                // the querier's side and the decryption (engine_query_steps.cpp): the launchers engine_query.cpp calls
                STEP_SEED_EXPAND, STEP_DECRYPT_ROUND, STEP_PLAIN_POWERS, STEP_SAMPLE_SMALL, STEP_SMALL_LIFT, STEP_ENC_FINISH, STEP_RLK_FINISH,
                STEP_FLAG_MONOMIAL,
                // the multiply-accumulate family (engine_mac_steps.cpp): the launchers of launch_mac.h and launch_limb0_rows
                STEP_MAC_INFO, STEP_MAC, STEP_TERM_PRODUCT, STEP_PACK_ROWS, STEP_UNPACK_ROWS, STEP_LIMB0_ROWS,
                // behind the existing ids, which stay: k_entries_scatter (engine_db_steps.cpp)
                STEP_ENTRIES_SCATTER,
                // the grouping by location (engine_bucket_steps.cpp): the per-kernel launchers of launch_bucket.h
                STEP_BUCKET_COUNT, STEP_BUCKET_KEYS, STEP_BUCKET_SCAN, STEP_BUCKET_HIST, STEP_BUCKET_SCATTER, STEP_BUCKET_OFFSETS, STEP_BUCKET_ORDER,
                STEP_ENTRIES_GATHER,
                // the launchers no other family reaches (engine_misc_steps.cpp): launch_ew.h's and launch_db.h's small ones
                STEP_ADD, STEP_CLEAR_BITS, STEP_COPY_JOBS, STEP_COPY_SOURCES, STEP_FILL_RANDOM, STEP_FILL_BLAKE2XB, STEP_SCATTER_SLOTS,
                STEP_GATHER_SLOTS, STEP_ALGEBRAIZE, STEP_PACK_BLOCKS, STEP_COUNT };
    enum : uint32_t { STEP_RAW = 1, STEP_ACCUMULATE = 2, STEP_STORE = 4, STEP_KEY = 8, STEP_PLAN = 16, STEP_COMPOSED = 32, STEP_INVERSE = 64, STEP_NORED = 128,
                      STEP_KARA = 256, STEP_PACKED = 512, STEP_LIMB_SLOW = 1024 };
    struct StepArgs {
        int step, chain_idx;
        uint32_t flags;
        int terms, polys, batch, e0, n_ext;
        const u64 *in[6];
        size_t in_words[6];
        u64 *out[2];
        size_t out_words[2];
    };
    void debug_run_step(const StepArgs &a);
    void debug_run_db_step(const StepArgs &a);                    // its database half (the caller holds the lock)
    void debug_run_ntt_step(const StepArgs &a);                   // its transform half (the caller holds the lock)
    void debug_run_query_step(const StepArgs &a);                 // its querier-side half (the caller holds the lock)
    void debug_run_mac_step(const StepArgs &a);                   // its multiply-accumulate half (the caller holds the lock)
    void debug_run_bucket_step(const StepArgs &a);                // its grouping half (the caller holds the lock)
    void debug_run_misc_step(const StepArgs &a);                  // the remaining launchers (the caller holds the lock)
    // Staging of apsu_he_run_query_request (c_api.cpp) kept across calls: a device buffer and a page-locked host buffer of at least
    // `bytes` (grown on demand; hipHostMalloc / hipMalloc per query cost milliseconds).  The caller holds wire_mutex() for the whole query.
    std::mutex &wire_mutex() { return wire_mu_; }
    void wire_stage(size_t bytes, u64 **device, u64 **pinned);

private:
    // arena (bump allocator reset per top-level operation)
    u64 *ws(size_t words);                                               // engine_impl.h
    template <class T> T *ws_as(size_t count, size_t extra_words = 0);   // engine_impl.h
    void ws_reset(size_t need_bytes_hint = 0);
    template <class T> const T *upload_jobs(const std::vector<T> &v);   // engine_impl.h

    const DevLevel *dlevel(int chain_idx) const { return d_levels_.u() ? reinterpret_cast<const DevLevel *>(d_levels_.p()) + chain_idx : nullptr; }
    const LevelConstants &hlevel(int chain_idx) const { return hp_.level[chain_idx]; }
    const NttTable *tabs() const { return reinterpret_cast<const NttTable *>(d_tabs_.p()); }
    const DevKey *dkey() const { return reinterpret_cast<const DevKey *>(d_key_.p()); }
    const int *map_ct() const { return reinterpret_cast<const int *>(d_map_ct_.p()); }
    const int *map_ext(int chain_idx) const { return reinterpret_cast<const int *>(d_map_ext_.p()) + chain_idx * DMAXE; }
    // the same map for the inverse transform in front of a finish kernel: NTT_MAP_RAW set where that level's finish takes
    // the twist into its own constants (behz_unrolled), identical to map_ext otherwise
    const int *map_ext_fin(int chain_idx) const { return reinterpret_cast<const int *>(d_map_ext_fin_.p()) + chain_idx * DMAXE; }
    const int *map_ks(int chain_idx) const { return reinterpret_cast<const int *>(d_map_ks_.p()) + chain_idx * (DMAXL + 1) * DMAXL; }
    const int *map_ksacc(int chain_idx) const { return reinterpret_cast<const int *>(d_map_ksacc_.p()) + chain_idx * (DMAXL + 1); }
    const int *map_ksacc_raw(int chain_idx) const { return reinterpret_cast<const int *>(d_map_ksacc_raw_.p()) + chain_idx * (DMAXL + 1); }

    // device-pointer building blocks
    // narrow: all moduli named by the map are narrow (data_primes_narrow_ / ext_primes_narrow_; ntt_form takes the launch's form from it)
    void d_ntt(u64 *data, size_t count, const int *modmap, int period, bool inverse, bool narrow);
    void d_ntt_ct(u64 *data, size_t polys, int chain_idx, bool inverse) { d_ntt(data, polys * (chain_idx + 1), map_ct(), chain_idx + 1, inverse, data_primes_narrow_); }
    // BFV multiply of `njobs` (a, b) pairs given as ext-NTT operands; writes size-3 results
    // ext_out / n_ext: the first n_ext ciphertexts also get their BEHZ extension written to ext_out[b][2][E][n] (fused into
    // the mod-down; returns false when the level has no unrolled extension and the caller must run launch_behz_ext itself)
    // defer_moddown (round 6): the caller's next kernel performs the rounding mod-down itself (k_eval_epilogue<true>): the RAW inverse transforms
    // of the key-switch sums are left at *defer_moddown ([batch][2][L+1][n], workspace) and ct3 is NOT updated.  Refused (nullptr stored) when the
    // level has no RAW mod-down constants (L > 4).
    bool d_relinearize(u64 *ct3, size_t ct_stride, int batch, const RelinKeys &rk, int chain_idx, u64 *ext_out = nullptr, int n_ext = 0,
                       u64 **defer_moddown = nullptr);
    void check_level(int chain_idx) const;
    // tier-1 caller data (host operands): every word of limb j of each of `polys` polynomials at chain_idx below q_j, else invalid_argument
    void check_tier1_residues(const u64 *ct, size_t polys, int chain_idx, const char *what) const;
    // BEHZ steps 4-8 for operands given as ext-NTT polynomials [size][E][n]; out: [sa + sb - 1][L][n], coefficient form
    void d_multiply_sized(const u64 *ea, int sa, const u64 *eb, int sb, u64 *out, int chain_idx);
    // ComputePowers / eval / eval_patstock without key switching and with products (ciphertexts of any size): plain
    // compositions of the per-polynomial kernels, not tuned -- no shipped parameter set reaches them
    std::unique_ptr<Powers> compute_powers_nks(const uint32_t *bundle_indices, int nb, const u64 *const *src, bool on_device);
    void eval_bundles_nks(const Bundle *const *bundles, int count, const Powers &pw, const u64 *const *masks, bool masks_on_device,
                          u64 *out, bool out_on_device, u64 *const *out_rows);
    PowerSizes sizes_;                // polynomials per target power; .products: no key switching AND the PowersDag has products
    uint32_t result_polys_ = 2;

    HeParams hp_;
    const EngineSwitches sw_ = read_switches();   // the environment, read once per context (dev_consts.h)
    PSUParams psu_;
    bool has_psu_ = false;
    PowersDag dag_;
    int device_ = 0;
    hipStream_t st_ = nullptr;
    std::mutex mu_;                   // ABI calls are serialised per context (thread-safe)

    DevBuf d_tabs_, d_tw_, d_levels_, d_key_, d_map_ct_, d_map_ext_, d_map_ext_fin_, d_map_ks_, d_map_ksacc_, d_map_ksacc_raw_, d_fin_, d_drop_, d_mdtw_;
    DevBuf arena_;
    size_t arena_off_ = 0;
    // Lanes: lane 0 = the main stream, lane 1 = a second stream with its own arena for work that is independent of
    // the main chain (the high-power half of ComputePowers).  st_/arena_/arena_off_/job_seq_ always describe the
    // CURRENT lane; switch_lane() parks them and loads the other lane's, so every helper works on either.
    struct Lane { hipStream_t st = nullptr; DevBuf arena; size_t off = 0, job_seq = 0; };
    Lane lanes_[3];                   // the lanes that are not current (the current one's state lives in st_ / arena_ / arena_off_ / job_seq_): 0 main,
                                      // 1 second stream (high-power chain; a queued query's whole ComputePowers), 2 the evaluation's side work
    int cur_lane_ = 0, overflow_lane_ = 0;
    void switch_lane(int lane);
    hipEvent_t ev_main_ = nullptr;    // main-stream progress marker the second stream waits on
    hipEvent_t ev_fork_ = nullptr, ev_side_ = nullptr, ev_intt_ = nullptr;   // eval_patstock's side lane: start marker on the main stream, end marker on the side stream, main-stream inverse transforms done
    bool inputs_ready_ = false;       // the caller's promise behind apsu_he_set_query_overlap: the second stream then waits for the last reader of its powers buffer only
    bool pipe_cp_ = true;             // queued queries: the whole ComputePowers on the second stream, next to the evaluation in front (set_query_overlap 1 / 3)
    bool force_pipe_ = false;         // ... whether or not an evaluation is still running (set_query_overlap 3)
    bool data_primes_narrow_ = false; // every key prime runs the transform without range control (ntt_is_narrow)
    bool ext_primes_narrow_ = false;  // ... and so does every modulus of the extended base q u Bsk (HeParams::aux_narrow)
    bool async_results_ = false;      // eval_bundles with device masks + device output returns once the work is queued
    // Asynchronous evaluations in flight: the host may run at most max_inflight_ queries ahead of the device.  Unbounded
    // run-ahead (20 queued queries = 1300 launches + 200 stream events) makes the HIP runtime block the host inside a
    // launch and drain its queues, which shows up as idle gaps on the device (profiles/r03_shard_probe.txt).
    std::vector<hipEvent_t> inflight_;
    size_t inflight_head_ = 0, inflight_count_ = 0;
    int max_inflight_ = 2;
    void throttle_inflight();
    void mark_inflight();
    // device-resident source ciphertexts are checked while they are gathered (k_copy_sources: every word below its limb's prime, SEAL's
    // is_data_valid_for); the kernel raises this word of page-locked host memory, sync() looks at it and throws std::invalid_argument
    // page-locked words written by k_copy_sources: slot (seq % BAD_SLOTS) holds the sequence number of the last ComputePowers that found
    // a source coefficient outside [0, q) there; bad_reported_ = what has been thrown already
    static constexpr int BAD_SLOTS = 16;
    unsigned *bad_source_ = nullptr;
    unsigned bad_reported_[BAD_SLOTS] = {};
    uint32_t query_seq_ = 0;
    void check_sources();                                         // any query
    void check_sources(const Powers &pw);                         // this query
    bool bad_source_pending(int slot, bool take);
    void *stage_ = nullptr;           // pinned host staging for job arrays
    size_t stage_bytes_ = 0, stage_off_ = 0;
    // job-array cache: the n-th upload of a top-level call usually carries the same bytes as in the
    // previous call of the same shape (workspace addresses are deterministic), so it is kept on the
    // device and the copy is skipped when the content hash matches.
    // Two ways per slot: a caller that still holds the previous query's powers while it computes the next one alternates
    // between two powers buffers, hence between two versions of every table that names them (tools/shard_probe.py).
    struct JobWay { DevBuf buf; std::vector<unsigned char> host; uint64_t stamp = 0; };
    struct JobSlot { JobWay way[4]; };                  // four-way: a stream of queries cycles through up to three powers buffers (compute_powers), whose addresses are in the tables
    uint64_t job_stamp_ = 0;
    std::vector<JobSlot> job_slots_;
    size_t job_seq_ = 0, job_seq_base_ = 0;   // slots [base, ..) belong to the running top-level op
    std::vector<std::unique_ptr<Powers>> powers_pool_;
public:
    void recycle_powers(std::unique_ptr<Powers> p);
private:
    std::vector<DevBuf> retired_;     // arenas replaced while kernels may still reference them
    uint64_t counters_[C_COUNT] = {};
    std::mutex wire_mu_;
    DevBuf wire_dev_;
    void *wire_pinned_ = nullptr;
    size_t wire_pinned_bytes_ = 0;

    // PowersDag schedules (powers_sched.h): the whole DAG's and, where split_ok_, its two halves' (empty where the
    // walk does not split)
    PowersSched sched_, sched_low_, sched_high_;
    void mask_generate_impl(uint32_t count, u64 *masks_dev, u64 *values_host, u64 *blocks_host, const std::function<void(u64 *, size_t)> &fill);
    bool fuse_tensor_ = true;         // BEHZ step 4 is formed by the inverse transform's load (k_intt_tensor); off only for n = 32768, whose limb does not fit one workgroup
    bool tier1_device_ = false;       // tier-1 operands are device memory and calls do not synchronise
    void tier1_done() { if (!tier1_device_ || prof_on_) sync(); }
    bool packed_rows_ = true;         // BinBundle plaintexts are kept bit-packed in HBM (EngineSwitches::packed_rows, with key switching only; Bundle::packed)
    // ---- the resident database (engine_bundles.cpp, engine_db.cpp); where a coefficient is stored: bundle_layout.h
    BundleLayout layout_of(uint32_t degree) const { return bundle_layout(psu_.query_params.ps_low_degree, degree, hp_.first_chain_idx); }
    std::unique_ptr<Bundle> new_bundle(uint32_t bundle_idx, uint32_t cache_idx, uint32_t degree, BundleLayout *layout = nullptr) const;   // the shape, no buffers yet
    size_t slot_bytes(int chain_idx, bool packed) const;          // bytes of one NTT-form plaintext at a level, either format
    void pack_bundle(Bundle &b);      // dense -> packed when this context keeps packed rows (no-op otherwise)
    void unpack_bundle(Bundle &b);    // packed -> dense (images of the other format)
    MacPlan plan_mac(const std::vector<MacStream> &streams, size_t nlimbs, size_t n) const;   // mac_plan.h with this context's primes and switch
    void d_mac(const MacPlan &p, const MacJob *jobs = nullptr);
    bool split_ok_ = false;           // the low-power and high-power halves of the PowersDag share no node
    int two_stream_mode_ = -1;        // apsu_he_set_two_stream (-1: EngineSwitches::two_stream_default)
    struct DagRun;                    // per-call state of one walk over a schedule
    void dag_sources(DagRun &run, const u64 *const *src, bool on_device);
    void dag_level(DagRun &run, size_t d, const RelinKeys *rk);
    void dag_outputs(DagRun &run, Powers &pw, bool do_low, bool do_high);
    void dag_walk(const PowersSched &s, int nb, const u64 *const *src, bool on_device, const RelinKeys *rk, Powers &pw);
    // what compute_powers and compute_powers_nks share: the Powers header of a new query (its sequence number included), and the
    // ComputePowers phase span around the walk -- body(span) runs inside WITH_ARENA and stamps the span's end(s) (engine_impl.h)
    void powers_header(Powers &pw, const uint32_t *bundle_indices, int nb, int low_level, int high_level);
    template <class F> void with_powers_span(F &&body);
    // eval_bundles in pieces (engine_eval.cpp): per-call context and Paterson-Stockmeyer batch; the plan: eval_plan.h
    struct EvalCall;
    void eval_plain(EvalCall &c, const std::vector<int> &pl_ids);
    void eval_patstock(EvalCall &c, const std::vector<int> &ps_ids);
    void ps_cf_streams(const EvalCall &c, const PsBatch &g, std::vector<MacStream> &out);
    void ps_cf_mac(const EvalCall &c, const PsBatch &g);
    void ps_term_product(const EvalCall &c, const PsBatch &g);
    void ps_i0_finish(const EvalCall &c, const EvalPlan &plan, const PsBatch &g, u64 *i0);
    void ps_tables(EvalCall &c, const EvalPlan &plan, PsBatch &g);
    void ps_run(EvalCall &c, const EvalPlan &plan, PsBatch &g);        // the steps below, in this order
    void ps_mac(EvalCall &c, const EvalPlan &plan, PsBatch &g);
    void ps_side(EvalCall &c, const EvalPlan &plan, PsBatch &g);
    void ps_drop_ext(EvalCall &c, const EvalPlan &plan, PsBatch &g);
    void ps_products_summed(EvalCall &c, const EvalPlan &plan, PsBatch &g);
    void ps_products_per_term(EvalCall &c, const EvalPlan &plan, PsBatch &g);
    u64 *ps_i0(EvalCall &c, const EvalPlan &plan, PsBatch &g);
    void ps_epilogue(EvalCall &c, PsBatch &g, const u64 *i0);
    // (engine_bundles.cpp: these three)
    void finish_bundle(Bundle &b, const u64 *raw);     // raw: [degree+1][n] coefficient-form plaintexts mod t (device)
    void encode_bundle(Bundle &b, const u64 *poly);    // poly: [degree+1][n] slot values -> BatchEncoder::encode, then finish_bundle
    // the inverse: the stored coefficients back to slot values [degree+1][n] mod t.  coeff (may be null): [degree+1][n], the coefficient
    // form mod t on the way there -- what BatchEncoder::encode made of each degree, before the forward transform mod t
    void decode_bundle(const Bundle &b, u64 *poly, u64 *coeff = nullptr);
    // its coefficient half: raw [degree+1][n] = what finish_bundle was given, the coefficient-form plaintexts mod t
    void decode_coeff(const Bundle &b, u64 *raw);
    // adopt_bundle's source side, under this context's lock: decode_coeff into a buffer of the call's own, complete on return
    void export_coeff(const Bundle &b, DevBuf &raw);
    // the tail of build_bundle: device root lists [bins][stride] and counts [bins] -> the stored BinBundle b (queued)
    void build_from_roots(Bundle &b, const u64 *droots, const uint32_t *dcounts, uint32_t bins, uint32_t stride);
    // ---- the calls on a resident database (engine_db.cpp, like everything from here to unlift_exact_)
    // The context's preconditions in their one order: PSUParams, batching, decodable stored plaintexts (q_0 > 2 t), each including the
    // ones before it; what (may be null): the call's name, for "more bins than batching slots"
    enum { NEED_PSU = 1, NEED_BATCHING, NEED_DECODE };
    void lookup_check(const char *what, int need = NEED_DECODE) const;
    // The prologue of every such call, inside its WITH_ARENA: poly [degree+1][n] from the arena = decode_bundle(b) (coeff as there), the
    // decode's workspace free again, then k_bin_counts into dcounts (device, n words; null: no counts).  evs (may be null): stamp `mid`
    // goes between the decode and the counts.
    u64 *decode_counted(const Bundle &b, uint32_t *dcounts, u64 *coeff = nullptr, EventStamps *evs = nullptr, size_t mid = 0);
    struct OpClock { EventStamps evs; double ms[OP_SPANS] = {}; } clock_[OP_COUNT];          // op_times
    // decode each BinBundle in turn through the arena; counts (may be null): [n_bundles][n]; flags (null when count == 0): [n_bundles][count * F]
    void lookup_impl(const Bundle *const *bundles, uint32_t n_bundles, const u64 *felts, const uint32_t *start, size_t count, uint32_t *counts,
                     unsigned char *flags);
    // bundles_eval_plain's and self_test's shared middle: queued inside the caller's WITH_ARENA; four time stamps per BinBundle from
    // evs[first] on, summed into ms[3] (decode, counts, kernel) by eval_plain_collect after the caller's sync
    void eval_plain_queue(const Bundle *const *bundles, uint32_t n_bundles, const u64 *const *xs, const u64 *const *masks, u64 *out, unsigned char *is_bin,
                          u32 *bad, EventStamps &evs, size_t first);
    static void eval_plain_collect(const EventStamps &evs, size_t first, uint32_t n_bundles, double *ms);
    // bundle_bins in stages, for export_saved to take the bins' rows and the coefficient-form plaintexts from the same decode between
    // (a) and (b), while the columns of poly are whole.  (a) and (b) run inside the caller's WITH_ARENA, (c) behind it.
    struct BinsCounted { u64 *poly, *coeff; uint32_t *dcounts; const uint32_t *counts; };      // device, device or null, device, host
    struct BinsFound { std::vector<uint32_t> occ, found, mult; std::vector<u64> hits; uint32_t hstride = 0; };
    bool bins_prepare(const Bundle &b, int form);      // the refusals and the context's tables; true: the persistent kernel
    // (a) decode, counts, the sync: stamps 0 and 1 of evs around them
    BinsCounted bins_counted(const Bundle &b, bool want_coeff, uint32_t *counts, EventStamps &evs);
    // (b) root search, stamp s, multiplicities and copies (queued), stamp s + 1.  stride (may be null): refused below the largest count
    void bins_search(const BinsCounted &c, bool kernel, const uint32_t *stride, EventStamps &evs, size_t s, BinsFound &f);
    // its device half: the launches alone (f.occ and f.hstride are set; null pointers where no bin is occupied), what they leave
    // on the device for launch_roots_split or for bins_search's three copies
    struct BinsDevice { uint32_t *occ, *found, *mult; u64 *hits; };
    BinsDevice bins_search_device(const BinsCounted &c, bool kernel, const uint32_t *stride, EventStamps &evs, size_t s, BinsFound &f);
    // (c) the host end: every bin's list checked and sorted, then written to roots (may be null)
    void bins_finish(const BinsCounted &c, BinsFound &f, u64 *roots, uint32_t stride);
    // the coefficient-form rows of decode_bundle's `coeff` that a saved BinBundle carries as they are: a_0, then the a_{i h} by slot
    void keep_coeff_rows(const Bundle &b, const u64 *coeff, DevBuf &keep);
    void roots_tables();                             // the context's generator, step table and point table, made by the first bundle_bins
    u64 roots_g_ = 0;
    DevBuf d_roots_step_, d_roots_pts_;                // g^i (u32) and the forward transform mod t of the polynomial X, n words each
    uint32_t scatter_blocks_ = 0;                      // set_scatter_blocks
    bool unlift_exact_ = false;                        // q_0 > 2 t (set at creation): a stored residue tells its value mod t (bin_update.h)
    DevBuf d_slot_map_;
    // ---- cuckoo hashing (engine_cuckoo.cpp)
    DevBuf d_cuckoo_tabs_;                             // [hash_func_count][16][256] words, made by the first call that hashes
    void cuckoo_tables_ready();
    const unsigned char *cuckoo_items(const unsigned char *items, size_t count, bool on_device);     // 16-byte aligned device memory (inside WITH_ARENA)
    struct BucketOut { u64 *offsets, *total; };        // device: [T + 1] and one word
    BucketOut bucket_run(const uint32_t *dlocs, size_t count, uint32_t H, uint32_t T, uint32_t tile, uint32_t *dorder);   // (inside WITH_ARENA)
    // inside the caller's WITH_ARENA: the launch, the status, then the copies to the host; throws for an unplaced item before any copy
    void cuckoo_insert_run(const unsigned char *ditems, const uint32_t *dlocs, uint32_t count, uint32_t H, uint32_t T, u64 max_rounds, int form,
                           uint32_t *table_idx, uint32_t *item_loc, u64 *rounds);
    // seed expansion of `count` objects of L limbs queued on the stream without a host wait (seed_expand, query_create, relin_keygen): false = the objects need the host's
    // sampler (seed_expand's rule) and nothing was queued; seeds_overflowed() after the final sync tells whether the device lists sufficed
    bool queue_seed_expand(int L, int count, const u64 *seeds, u64 *const *dst);
    bool seeds_overflowed(int count);
    const DevLevel *seed_level(int L);                // the level block an expansion of L limbs reads: a data level's, or the key level's view (uploaded by the first use)
    void host_seed_expand(int L, int count, const u64 *seeds, u64 *const *dst);
    void check_key_residues(const u64 *sk_ntt_host, int limbs) const;
    // seed expansion: rejection lists; the DevLevel-shaped view of the key level and max_multiple per key prime as build_device_constants
    // made them.  The view is uploaded by the first expansion at the key level, not at creation: one more allocation in front of the
    // database upload would move every buffer behind it (k_mac's rate depends on where they land).
    DevBuf d_seed_rej_, d_key_level_;
    std::vector<DevLevel> key_level_;
    std::vector<u64> max_multiple_;

    // profiling state
    struct ProfRec { hipEvent_t a, b; int kind; uint64_t units; };
    bool prof_on_ = false, prof_open_ = false, prof_ntt_only_ = false;
    std::vector<ProfRec> prof_recs_;
    std::vector<hipEvent_t> prof_pool_;
    ProfStats prof_{};
    void prof_begin(int kind, uint64_t units);
    void prof_end();
    void prof_collect();

    // phase timers
    struct PhaseSpan { hipEvent_t a = nullptr, b = nullptr, b2 = nullptr; int phase = 0; };
    bool phase_on_ = false;
    std::vector<PhaseSpan> phase_spans_;
    std::vector<hipEvent_t> phase_pool_;
    PhaseSummary phase_[PH_COUNT];
    hipEvent_t query_start_ = nullptr, query_end_ = nullptr;     // the open RunQuery span
    hipEvent_t phase_event(hipStream_t st);
    void phase_close_query();
    void phase_collect();
    struct Enter;                     // lock + current-device guard taken by every public entry point (engine_impl.h)
    friend struct EngineAccess;
    friend struct ProfScope;
};

} // namespace apsu_he
