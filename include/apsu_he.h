/*
 * apsu_he.h — C ABI of the MI355X homomorphic query-evaluation engine for APSU.
 *
 * Drop-in boundary: these entry points replace the seal::Evaluator calls that the DB-holding
 * party (apsu::receiver::Receiver) makes on its hot path.  The reference has no FFI for this
 * path; the replaced interface is the C++ class seal::Evaluator reached through
 * CryptoContext::evaluator() (common/apsu/crypto_context.h:101-104).  Each function below
 * cites the reference call site(s) it replaces.  INTEGRATION.md shows the adapter a maintainer
 * adds to receiver/apsu/receiver_osn.cpp and receiver/apsu/bin_bundle.cpp.
 *
 * Conventions
 *  - Buffers are raw uint64_t limb arrays in SEAL's in-memory order [poly][limb][coeff], i.e.
 *    exactly Ciphertext::data() / Plaintext::data().
 *  - Levels are named by SEAL's chain_index (0 = last level); get_parms_id_for_chain_idx
 *    (common/apsu/util/utils.cpp:179-189) gives the mapping on the SEAL side.
 *  - Every function returns 0 on success or a negative apsu_he_status; the message of the last
 *    failure on the calling thread is available from apsu_he_last_error().  C++ callers map
 *    APSU_HE_INVALID_ARGUMENT -> std::invalid_argument, others -> std::runtime_error, which is
 *    what the reference's callers see from SEAL (bin_bundle.cpp:116-118,204-213).
 *  - All-zero operands are legal (SEAL_THROW_ON_TRANSPARENT_CIPHERTEXT=OFF, bin_bundle.cpp:111-114).
 *  - Calls on one context are thread-safe (serialised internally); the reference calls the
 *    Evaluator from a thread pool (receiver_osn.cpp:334-364).
 *  - There is NO CPU fallback: apsu_he_create fails with APSU_HE_NO_DEVICE without a GPU.
 */
#ifndef APSU_HE_H
#define APSU_HE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    APSU_HE_OK = 0,
    APSU_HE_INVALID_ARGUMENT = -1,   /* std::invalid_argument in the reference */
    APSU_HE_LOGIC_ERROR = -2,        /* std::logic_error */
    APSU_HE_RUNTIME_ERROR = -3,      /* std::runtime_error (incl. HIP failures) */
    APSU_HE_NO_DEVICE = -4,          /* no MI355X / HIP device visible */
    APSU_HE_OUT_OF_MEMORY = -5
} apsu_he_status;

typedef struct apsu_he_ctx apsu_he_ctx;         /* CryptoContext + Evaluator replacement */
typedef struct apsu_he_relin apsu_he_relin;     /* device-resident seal::RelinKeys */
typedef struct apsu_he_bundle apsu_he_bundle;   /* device-resident BinBundleCache::batched_matching_polyn */
typedef struct apsu_he_powers apsu_he_powers;   /* device-resident CiphertextPowers for some bundle indices */

typedef struct {
    uint64_t poly_modulus_degree;
    uint64_t plain_modulus;
    int32_t coeff_modulus_size;      /* K, limbs at key level */
    int32_t first_chain_idx;         /* chain_index of the first data level */
    int32_t using_keyswitching;
    int32_t irrelevant_bit_count;    /* bin_bundle.cpp:67-97 */
    uint64_t coeff_modulus[8];
    /* PSUParams-derived (zero when created without PSUParams) */
    uint32_t ps_low_degree, max_items_per_bin, bundle_idx_count, items_per_bundle;
    uint32_t source_power_count, target_power_count, powers_dag_depth;
    uint32_t result_polys;           /* polynomials per row of apsu_he_eval_bundles' output: 2 with key switching; more only for
                                      * parameter sets with ONE coefficient prime, whose products are never relinearised
                                      * (receiver_osn.cpp:416,430-432 ; bin_bundle.cpp:238-240,308-310)   (ABI 4; was `reserved`) */
} apsu_he_info;

typedef struct { uint32_t power, depth, parent1, parent2; } apsu_he_dag_node;   /* powers.h:53-77 */

const char *apsu_he_last_error(void);
/* 1: tiers 1 and 2, N1, N2, N4.  2 (additive): apsu_he_multi_*, apsu_he_eval_all, apsu_he_partition_bundles, apsu_he_wire_*,
 * apsu_he_set_async_results / apsu_he_sync / apsu_he_stream, apsu_he_mask_generate_blake2xb.
 * 6: apsu_he_set_query_overlap.  7: its modes 2 and 3; the APSU_HE_* environment switches of measured-and-decided A/B experiments are gone.
 * 3: apsu_he_set_eval_pipeline removed (measured-negative scheduling experiment, profiles/r03_eval_pipeline.txt); added
 * apsu_he_debug_counters, apsu_he_phase_* / apsu_he_multi_phase_*, apsu_he_eval_all_ex + apsu_he_host_alloc, apsu_he_partition_bundles_ex,
 * the SEAL object codec apsu_he_seal_*, apsu_he_seed_expand, apsu_he_run_query_request; poly_modulus_degree 32768.
 * 4 (additive): ciphertexts of more than two polynomials for parameter sets without key switching -- apsu_he_multiply_sized,
 * apsu_he_power_size, apsu_he_bundle_result_size, apsu_he_info.result_polys (the former `reserved`); those sets were refused before.
 * apsu_he_algebraize_items (N1: item -> field elements); apsu_he_db_file_* / apsu_he_multi_db_load_file / _save_file (N2: the whole DB
 * in one mmap-able file); apsu_he_seal_pt_load / _save, apsu_he_db_upload_bundle_serialized (BinBundle caches as the reference stores
 * them), apsu_he_db_upload_saved_bundle (a BinBundle as ReceiverDB::save wrote it); zstd bodies in the SEAL codec;
 * apsu_he_multi_run_query_request, apsu_he_multi_result_polys; the parameter exchange, plainResponse, PSUParams in binary form and
 * the header of a saved ReceiverDB (apsu_he_wire_peek_type ... apsu_he_wire_receiver_db_header).
 * 5 (additive): apsu_he_set_tier1_on_device (tier-1 calls on device-resident operands without a host round trip per call);
 * BinBundle images and DB files carry a row format (bit-packed database rows, the default, or dense words) and load into either. */
#define APSU_HE_ABI_VERSION 7   /* what this header describes; compare with apsu_he_abi_version() of the loaded library */
int apsu_he_abi_version(void);

/* ---- lifetime ------------------------------------------------------------------------------ */
/* PSUParams::Load(json) + CryptoContext(params) (psu_params.cpp:290-374, crypto_context.h:32-37) */
int apsu_he_create(const char *psu_params_json, int device, apsu_he_ctx **out);
/* SEALContext from explicit primes (tests / tier-1 use without PSUParams).  Each prime has at most 60 bits
 * (SEAL_USER_MOD_BIT_COUNT_MAX), as coeff_modulus_bits of the JSON form: a wider one is APSU_HE_INVALID_ARGUMENT. */
int apsu_he_create_raw(uint64_t poly_modulus_degree, const uint64_t *coeff_modulus, int coeff_modulus_size,
                       uint64_t plain_modulus, int device, apsu_he_ctx **out);
int apsu_he_destroy(apsu_he_ctx *ctx);
int apsu_he_get_info(const apsu_he_ctx *ctx, apsu_he_info *out);
/* PowersDag::configure result (powers.cpp:22-107); nodes ascending by power. Returns count via *n_nodes. */
int apsu_he_get_powers_dag(const apsu_he_ctx *ctx, apsu_he_dag_node *nodes, int capacity, int *n_nodes);

/* ---- tier 1: one call per Evaluator method (host buffers) ---------------------------------- */
/* Evaluator::transform_to_ntt_inplace(Ciphertext)        receiver_osn.cpp:467,475 */
int apsu_he_transform_to_ntt(apsu_he_ctx *ctx, uint64_t *ct, int polys, int chain_idx);
/* Evaluator::transform_from_ntt_inplace                  bin_bundle.cpp:154,268,297,321 */
int apsu_he_transform_from_ntt(apsu_he_ctx *ctx, uint64_t *ct, int polys, int chain_idx);
/* Evaluator::transform_to_ntt_inplace(Plaintext, parms)  bin_bundle.cpp:419 ; out: (chain_idx+1)*n words */
int apsu_he_transform_plain_to_ntt(apsu_he_ctx *ctx, const uint64_t *pt_mod_t, size_t pt_coeff_count, uint64_t *out,
                                   int chain_idx);
/* Evaluator::multiply_plain, NTT ct x NTT plaintext      bin_bundle.cpp:147,258,287,320 */
int apsu_he_multiply_plain_ntt(apsu_he_ctx *ctx, const uint64_t *ct, const uint64_t *pt_ntt, uint64_t *out, int polys,
                               int chain_idx);
/* Evaluator::multiply_plain, coefficient ct x coefficient plaintext   bin_bundle.cpp:334 */
int apsu_he_multiply_plain(apsu_he_ctx *ctx, const uint64_t *ct, const uint64_t *pt_mod_t, size_t pt_coeff_count,
                           uint64_t *out, int polys, int chain_idx);
/* Evaluator::add_inplace                                  bin_bundle.cpp:148,264,273,293,303,323,336 */
int apsu_he_add(apsu_he_ctx *ctx, uint64_t *acc, const uint64_t *x, int polys, int chain_idx);
/* Evaluator::add_plain_inplace (adds to c0)               bin_bundle.cpp:159,162,345,346 */
int apsu_he_add_plain(apsu_he_ctx *ctx, uint64_t *ct, const uint64_t *pt_mod_t, size_t pt_coeff_count, int chain_idx);
/* Evaluator::multiply / multiply_inplace (size 2 x size 2 -> size 3)   receiver_osn.cpp:424 ; bin_bundle.cpp:272,301 */
int apsu_he_multiply(apsu_he_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *out3, int chain_idx);
/* Evaluator::square                                        receiver_osn.cpp:422 */
int apsu_he_square(apsu_he_ctx *ctx, const uint64_t *a, uint64_t *out3, int chain_idx);
/* Evaluator::multiply for operands that were never relinearised (one coefficient prime: receiver_osn.cpp:424 with :430-432
 * skipped ; bin_bundle.cpp:272,301): out has size_a + size_b - 1 polynomials; APSU_HE_INVALID_ARGUMENT beyond SEAL's largest
 * ciphertext (16 polynomials), where SEAL throws */
int apsu_he_multiply_sized(apsu_he_ctx *ctx, const uint64_t *a, int size_a, const uint64_t *b, int size_b, uint64_t *out, int chain_idx);
/* Evaluator::relinearize_inplace (size 3 -> size 2, in place in the first two polys)
 *                                                          receiver_osn.cpp:431 ; bin_bundle.cpp:309 */
int apsu_he_relinearize(apsu_he_ctx *ctx, uint64_t *ct3, const apsu_he_relin *rk, int chain_idx);
/* Evaluator::mod_switch_to_next_inplace; result packed [polys][chain_idx][n] at the front of ct
 *                                                          receiver_osn.cpp:463,471,478 ; bin_bundle.cpp:169,269,298,322,355 */
int apsu_he_mod_switch_to_next(apsu_he_ctx *ctx, uint64_t *ct, int polys, int chain_idx);
/* try_clear_irrelevant_bits (last level, one limb)         bin_bundle.cpp:67-97 */
int apsu_he_clear_irrelevant_bits(apsu_he_ctx *ctx, uint64_t *ct_last_level, int polys);

/* ---- tier 2: fused, HBM-resident ------------------------------------------------------------ */
/* RelinKeys of the query: [decomp K-1][component 2][limb K][n] = key_vector[J].data() of
 * KSwitchKeys::data()[0], NTT form (query.cpp:46-52, crypto_context.h:45-49) */
int apsu_he_relin_upload(apsu_he_ctx *ctx, const uint64_t *ksk, apsu_he_relin **out);
int apsu_he_relin_free(apsu_he_relin *rk);
/* BatchedPlaintextPolyn ctor output (bin_bundle.cpp:366-430): coeff_ptrs[d] = Plaintext::data() of
 * batched_coeffs[d]; is_ntt[d] per the rule at :418-420 (checked).  NTT-form plaintexts have
 * (plain_level+1)*n words, coefficient-form ones n words.  The engine copies; caller may free.
 * Called from ReceiverDB::generate_caches (receiver_db.cpp:808-820). */
int apsu_he_db_upload_bundle(apsu_he_ctx *ctx, uint32_t bundle_idx, uint32_t cache_idx, uint32_t n_coeffs,
                             const uint64_t *const *coeff_ptrs, const uint8_t *is_ntt, apsu_he_bundle **out);
/* Synthetic BinBundle for benchmarks: coefficient d, index k of the batched polynomial (coefficient
 * form, mod t) = splitmix64_mix(seed + (d*n + k + 1) * 0x9e3779b97f4a7c15) % t; generated on the GPU. */
int apsu_he_db_random_bundle(apsu_he_ctx *ctx, uint32_t bundle_idx, uint32_t cache_idx, uint32_t degree, uint64_t seed,
                             apsu_he_bundle **out);
/* "next" row N1: BinBundle::regen_polyns + regen_plaintexts on the GPU
 * (bin_bundle.cpp:934-1026 -> polyn_with_roots, common/apsu/util/interpolate.cpp:63-80 -> BatchedPlaintextPolyn
 * ctor bin_bundle.cpp:366-430: BatchEncoder::encode, transform_to_ntt).  roots[bin*stride + r], r < counts[bin],
 * are the field elements (mod plain_modulus) stored in bin `bin`; bins <= poly_modulus_degree; empty bins give the
 * polynomial 1.  The result is identical to uploading the reference-built cache with apsu_he_db_upload_bundle. */
int apsu_he_db_build_bundle(apsu_he_ctx *ctx, uint32_t bundle_idx, uint32_t cache_idx, const uint64_t *roots,
                            const uint32_t *counts, uint32_t bins, uint32_t stride, apsu_he_bundle **out);
/* N1, the update: insert items into and remove items from single bins of a resident BinBundle, the GPU side of
 * ReceiverDB::insert_or_assign / remove (receiver_db.cpp:330-433 -> BinBundle::multi_insert / try_multi_remove -> regen_cache).
 * ins_roots[bin*ins_stride + r], r < ins_counts[bin], and rem_roots / rem_counts / rem_stride likewise, follow the conventions of
 * apsu_he_db_build_bundle; either list may be NULL together with its counts (nothing of that kind).  `old` needs no roots behind
 * it: a built, uploaded, loaded (image, DB file, reference-saved) or already updated BinBundle will do.
 *  - The polynomial of bin (slot) s is whatever `old` holds there; its count is the index of its highest non-zero coefficient.
 *  - Remove: P <- P / (x - r), once per listed root.  The remainder must be 0: otherwise APSU_HE_INVALID_ARGUMENT, apsu_he_last_error
 *    names the first bin (lowest slot) and the root for which it was not, and no bundle is produced.  Removals come before insertions,
 *    so removing and inserting the same value is the identity.
 *  - Insert: P <- P (x - r) mod plain_modulus, once per listed root; the list is a multiset.
 *  - A slot holding the zero polynomial is not a bin (the build writes 0 beyond `bins`): a non-empty list for it is an error.  An
 *    empty bin holds the polynomial 1 and may be inserted into.
 *  - Refused as by the build: a root >= plain_modulus, bins > poly_modulus_degree, a resulting count above max_items_per_bin, a
 *    context without PSUParams or without batching (and one whose first coefficient prime is not above 2 * plain_modulus).
 *  - *out is a NEW bundle with old's bundle_idx and cache_idx; its degree is the largest resulting count (it may grow or shrink), and
 *    level, Paterson-Stockmeyer layout, monomial flags and row packing follow from it as in the build.  `old` is only read and stays
 *    valid until the caller frees it (queued evaluations may still read it).
 *  - If old = build_bundle(B), the image of the result (apsu_he_bundle_save) is byte-identical to that of build_bundle(B') for the
 *    updated bins B', in whatever order the roots are listed.
 * Synchronous.  apsu_he_multi_db_update_bundle replaces BinBundle `id` of a multi-device handle on its device, under the handle's
 * placement lock; the BinBundle keeps its id and therefore its row in apsu_he_eval_all. */
int apsu_he_bundle_update(apsu_he_ctx *ctx, const apsu_he_bundle *old, const uint64_t *ins_roots, const uint32_t *ins_counts,
                          uint32_t ins_stride, const uint64_t *rem_roots, const uint32_t *rem_counts, uint32_t rem_stride,
                          uint32_t bins, apsu_he_bundle **out);
/* N1, find and place: the database-level step above apsu_he_bundle_update.  What the reference keeps on the host next to a BinBundle
 * -- item_bins_, the cuckoo filters, hashed_items_ -- is asked of the resident polynomials instead, so a database that came from an
 * image, a DB file or a reference-saved cache can have items inserted and removed without anybody knowing its bins.
 * An ENTRY is what preprocess_unlabeled_data emits per cuckoo location (receiver_db.cpp:292-299): felts_per_item field elements
 * f_0 .. f_{F-1} (each < plain_modulus) and a start bin s, s + F <= bins_per_bundle; part j belongs to bin s + j.  The OPRF stays
 * with the caller; the cuckoo locations and their entries are apsu_he_items_bucket's, the field elements apsu_he_algebraize_items'.
 *  - A bin's COUNT is the index of the highest non-zero coefficient of its polynomial (the update's definition).  A slot that holds
 *    the zero polynomial is not a bin: APSU_HE_NOT_A_BIN.
 *  - An entry is PRESENT in a BinBundle iff P_{s+j}(f_j) = 0 mod plain_modulus for every j and every s + j is a bin.  That is
 *    try_multi_remove's test part by part, and what the protocol itself detects.  It includes the reference's false positive: every
 *    part present in its bin, each from a different item.
 * apsu_he_bundle_bin_counts: counts[poly_modulus_degree] (host) of one BinBundle.
 * apsu_he_bundles_lookup: felts[count][F], start_bins[count] against n_bundles BinBundles; present[n_bundles][count] (0 / 1) and
 * room[n_bundles][count] = max_j(count of bin s + j, + 1), the value of BinBundle::multi_insert_dry_run, or APSU_HE_NOT_A_BIN where
 * some slot is not a bin.  Either output may be NULL.  The BinBundles are decoded and looked up one after the other through the
 * context's workspace (k_bins_lookup: Horner evaluation with lane = slot, every stored coefficient read once per 8 points of its 64
 * slots); the work is bounded by the number of parts however they are spread over the bins.
 * apsu_he_db_apply_entries applies a batch to the BinBundles of ONE bundle index, given in cache order (ascending cache_idx; a
 * BinBundle of another bundle index, or out of order: APSU_HE_INVALID_ARGUMENT): lookup, the reference's placement rule, then
 * apsu_he_bundle_update per changed BinBundle and apsu_he_db_build_bundle per appended one.
 *  - Removals come first, as in the update.  An entry leaves the first BinBundle in cache order that holds it (receiver_db.cpp:543-549):
 *    APSU_HE_ENTRY_REMOVED, target = its position in `bundles`.  Held by none: APSU_HE_ENTRY_NOT_FOUND, nothing happens for it.
 *  - Insertions follow in list order, as ReceiverDB::insert_or_assign runs them (receiver_db.cpp:349-434).  An entry that is present in
 *    any of the BinBundles (before this call's changes), or equal to one placed earlier in the same call, is APSU_HE_ENTRY_DUPLICATE
 *    (target: where it is) -- the role of hashed_items_.  Otherwise the BinBundles are tried newest first; the entry fits iff every
 *    s + j is a bin and max_j(count + 1) < max_items_per_bin, strictly, so bins never exceed max_items_per_bin - 1.  Counts follow the
 *    entries placed before it and this call's removals.  An entry that fits nowhere opens a new BinBundle, which is the newest for the
 *    entries behind it.  APSU_HE_ENTRY_INSERTED, target = position in `bundles`, or n_bundles + k for the k-th appended BinBundle.
 *  - Refused as a whole (APSU_HE_INVALID_ARGUMENT, no handle is produced): an entry in both lists, an entry twice in the removal list,
 *    a part >= plain_modulus, s + F > bins_per_bundle.  Two removals that name the same value of the same bin are both scheduled; if
 *    the bin holds it only once, the update's division refuses the call ("is not a root").
 *  - bundle_state[i]: APSU_HE_BUNDLE_UNCHANGED (replaced[i] = NULL), _REPLACED (replaced[i] = a NEW bundle with the old one's bundle_idx
 *    and cache_idx) or _EMPTY: every bin count is 0 after the removals -- no handle is produced (replaced[i] = NULL), the caller drops
 *    the BinBundle as receiver_db.cpp:551-555 does, and it takes no insertion of this call.  The given handles are only read and stay
 *    valid, as with the update.  Surviving BinBundles keep their cache_idx (the reference renumbers by position).
 *  - appended[k], k < *n_appended <= n_ins: the new BinBundles, cache_idx continuing above the largest given (from 0 when none is given).
 *  - ins_status / ins_target [n_ins], rem_status / rem_target [n_rem] may each be NULL.  Target of NOT_FOUND: APSU_HE_NOT_A_BIN.
 * Preconditions and locking are the update's (PSUParams, batching, first coefficient prime above 2 * plain_modulus; synchronous; the
 * context's lock is taken per step).  The multi-device handle has its own form, apsu_he_multi_db_apply_entries. */
#define APSU_HE_NOT_A_BIN 0xFFFFFFFFu
enum { APSU_HE_ENTRY_INSERTED = 0, APSU_HE_ENTRY_DUPLICATE = 1, APSU_HE_ENTRY_REMOVED = 2, APSU_HE_ENTRY_NOT_FOUND = 3 };
enum { APSU_HE_BUNDLE_UNCHANGED = 0, APSU_HE_BUNDLE_REPLACED = 1, APSU_HE_BUNDLE_EMPTY = 2 };
int apsu_he_bundle_bin_counts(apsu_he_ctx *ctx, const apsu_he_bundle *bundle, uint32_t *counts);
int apsu_he_bundles_lookup(apsu_he_ctx *ctx, const apsu_he_bundle *const *bundles, uint32_t n_bundles, const uint64_t *felts,
                           const uint32_t *start_bins, size_t count, uint8_t *present, uint32_t *room);
int apsu_he_db_apply_entries(apsu_he_ctx *ctx, uint32_t bundle_idx, const apsu_he_bundle *const *bundles, uint32_t n_bundles,
                             const uint64_t *ins_felts, const uint32_t *ins_start, size_t n_ins, const uint64_t *rem_felts,
                             const uint32_t *rem_start, size_t n_rem, uint32_t *bundle_state, apsu_he_bundle **replaced,
                             apsu_he_bundle **appended, uint32_t *n_appended, uint32_t *ins_status, uint32_t *ins_target,
                             uint32_t *rem_status, uint32_t *rem_target);
/* device time of the context's last call of the three above, summed over its BinBundles: the decode, and the kernels behind it */
int apsu_he_debug_lookup_times(apsu_he_ctx *ctx, double *decode_ms, double *kernels_ms);
/* N1, a whole database from its entries in one call: ReceiverDB::set_data, which is clear plus the insertion loop on an EMPTY database
 * (receiver_db.cpp:349-434).  apsu_he_db_apply_entries is the incremental path: it looks every entry up and places it on the host, one
 * by one.  From empty that loop has a closed form, because the bins of two cuckoo locations of one bundle index never overlap (location
 * l owns bins (l % items_per_bundle) F .. + F - 1): "BinBundles newest first, strictly below max_items_per_bin, else a new one"
 * reduces to one running number per bundle index.
 *  - cap = max_items_per_bin - 1 entries of one location fit one BinBundle.  K_l = the BinBundles of l's bundle index when location l
 *    begins = the largest ceil(c_l' / cap) over the earlier locations l' of that index (c = entries of a location).  Entry i of
 *    location l, 0-based in list order, is in chunk m = i / cap; it goes to BinBundle K_l - 1 - m if m < K_l, else to BinBundle m, at
 *    position i - m cap of its bins.  The BinBundles of an index are numbered from 0 in the order the loop opens them: cache_idx = k, as
 *    apsu_he_db_apply_entries numbers BinBundles appended to an empty index.
 *  - entries [offsets[table_size]][16]: the post-OPRF items in apsu_he_items_bucket's order (the OPRF runs per location between the
 *    bucketing and this call, receiver_db.cpp:290-299), host memory or, with entries_on_device, device memory of the context's device;
 *    offsets [table_size + 1]: host.  Per bundle index its entries are copied once; per BinBundle one kernel (k_entries_scatter) splits
 *    every item into its field elements (apsu_he_algebraize_items' rule) and writes them into the BinBundle's root lists on the device,
 *    which the build consumes there.  No entry is touched on the host and no host-side copy of the bins exists.
 *  - NO entry-level dedupe: the reference's loop has none (hashed_items_ dedupes ITEMS before the OPRF).  Two equal entries of one
 *    location put a double root into their bins, and the result is apsu_he_db_build_bundle of bins that hold that root twice.  For
 *    lists whose entries are distinct per location the result is, byte for byte (apsu_he_bundle_save), what apsu_he_db_apply_entries
 *    appends per bundle index when it starts from no BinBundle.
 *  - apsu_he_db_entries_plan: the host half alone.  bundles_per_index [bundle_idx_count] (may be NULL), *total their sum.
 *  - apsu_he_db_build_from_entries: out[i], i < *n_out = the plan's total, bundle index by bundle index, in cache order within each; a
 *    bundle index without entries gets no BinBundle.  capacity below the total: APSU_HE_INVALID_ARGUMENT with the needed count in the
 *    error text (and in *n_out), nothing built.  All or nothing: on any failure no handle is produced.
 *  - Refused (APSU_HE_INVALID_ARGUMENT): offsets that decrease, a location with more than 2^32 - 1 entries, max_items_per_bin < 2
 *    (cap would be 0).  Preconditions: PSUParams and batching.  Synchronous.
 *  - The step in front of this call on the device as well: apsu_he_items_bucket_device leaves the entries in device memory in exactly
 *    the order this call reads, so that with an OPRF that runs on the device (or none) a database goes from items to resident
 *    BinBundles with nothing but offsets visiting the host.
 * Out of scope: building onto a bundle index that already has BinBundles (the incremental call's).
 * apsu_he_debug_build_from_entries_times: device time of the context's last such call, summed over bundle indices and BinBundles: the
 * entries' copies, k_entries_scatter, the builds.
 * apsu_he_debug_set_scatter_blocks (measurements): workgroups per location of k_entries_scatter in the calls that follow; 0, the
 * default, = one per 256 entries of a full chunk, fewer where the grid would pass about 16384 workgroups.  The results do not depend on it. */
int apsu_he_db_entries_plan(const apsu_he_ctx *ctx, const uint64_t *offsets, uint32_t *bundles_per_index, uint32_t *total);
int apsu_he_db_build_from_entries(apsu_he_ctx *ctx, const uint8_t *entries, int entries_on_device, const uint64_t *offsets,
                                  apsu_he_bundle **out, uint32_t capacity, uint32_t *n_out);
int apsu_he_debug_build_from_entries_times(apsu_he_ctx *ctx, double *copy_ms, double *scatter_ms, double *build_ms);
int apsu_he_debug_set_scatter_blocks(apsu_he_ctx *ctx, uint32_t blocks);
/* N1, reading the bins back: the items of a resident BinBundle, read from its polynomials -- the one question apsu_he_bundles_lookup
 * cannot answer, since it takes values the caller already knows.  With it a database that came from an image, a DB file or a
 * reference-saved cache can be rebuilt for other parameters (apsu_he_db_build_bundle of the bins in another context), audited, or counted
 * with exact multiplicities (the root test of the lookup cannot count them).
 *  - counts[poly_modulus_degree]: items in bin s as apsu_he_bundle_bin_counts gives them, APSU_HE_NOT_A_BIN for a slot holding the zero
 *    polynomial.
 *  - roots[poly_modulus_degree * stride], may be NULL to get only the counts (the bins are found and checked all the same): bin s at
 *    roots[s * stride], ascending, a value of multiplicity m written m times.  Words past a bin's count and rows of slots that are not
 *    bins are left alone.
 * For b = apsu_he_db_build_bundle(B), any update or merge of such BinBundles, and the same BinBundle loaded from an image or a DB file:
 * the bins equal B bin by bin as sorted multisets, and apsu_he_db_build_bundle of them gives a byte-identical image.
 * How: batching forces plain_modulus t = 1 (mod 2n), and the forward negacyclic transform mod t evaluates a polynomial at one coset of
 * the subgroup of order n of F_t^*.  Scaling coefficient i by g^(j i) for a generator g moves it to coset j; the (t - 1) / n cosets tile
 * F_t^*.  A bin's roots are the zeros of (t - 1) / n transforms (one workgroup per bin, persistent over the cosets, the bin's coefficients
 * resident in LDS: k_bin_roots) plus a_0 = 0 for the root 0; multiplicities by the first derivative, and division where it vanishes.
 * Refusals (nothing is written past the counts):
 *  - roots given and stride below the largest count: APSU_HE_INVALID_ARGUMENT.
 *  - a bin whose roots, counted with multiplicity, do not sum to its count: APSU_HE_INVALID_ARGUMENT; apsu_he_last_error names the first
 *    such slot, its count and the number found.  Such a polynomial is not a product of linear factors: apsu_he_db_random_bundle makes
 *    one, and so does a damaged image.
 *  - (t - 1) / n > 65536: APSU_HE_LOGIC_ERROR, stating t and the coset count.  A property of the context, like q_0 <= 2 * plain_modulus;
 *    every shipped parameter file stays under it (the largest has 8192 cosets).  A degree of poly_modulus_degree or more: likewise.
 * Preconditions and locking are apsu_he_bundle_bin_counts's.  Synchronous; the BinBundle is only read.
 * apsu_he_debug_bundle_bins_form: the same with the path named (0: the context's choice; 1: k_bin_roots, APSU_HE_LOGIC_ERROR for a ring
 * size without one; 2: the per-coset composition gather + library transform + scan that serves those ring sizes) -- for the tests that
 * hold the two against each other.  apsu_he_debug_bins_times: device time of the context's last such call: decode and counts, the root
 * search, multiplicities and copy-back. */
int apsu_he_bundle_bins(apsu_he_ctx *ctx, const apsu_he_bundle *bundle, uint64_t *roots, uint32_t *counts, uint32_t stride);
int apsu_he_debug_bundle_bins_form(apsu_he_ctx *ctx, const apsu_he_bundle *bundle, uint64_t *roots, uint32_t *counts, uint32_t stride, int form);
int apsu_he_debug_bins_times(apsu_he_ctx *ctx, double *decode_ms, double *roots_ms, double *mult_ms);
/* One element-wise kernel on caller-chosen words (added after ABI 7, additive; the ABI stays 7).  TEST-ONLY, synchronous, not for
 * callers: it exists for the tests that hold each kernel against a big-integer model of the same step at the inputs where the
 * kernel's range argument is tight -- inputs no public call can steer, since in a query they come out of transforms and base
 * conversions.  The call copies the host arrays to the device, builds the job structs, calls the very launch function the engine
 * calls for that step with the context's own constant blocks of chain level chain_idx (so the launcher's choice of kernel is part of
 * what runs), waits, and copies the result back.  Layouts ([..][n] words, n = poly_modulus_degree; L limbs at chain_idx, nB auxiliary
 * primes, nBsk = nB + 1, E = L + nBsk, K key primes; `batch` jobs):
 *   LEVEL_INFO      out[0] = L, nB, unrolled (L == nB <= 3), K, q_0 .., B_0 .., m_sk, special prime (0 without key switching),
 *                   irrelevant_bit_count -- the moduli the model needs (the auxiliary base is the engine's own choice)
 *   BEHZ_EXT        in[0] [batch][polys][L][n] -> out[0] [batch][polys][E][n]
 *   DROP_BEHZ_EXT   in[0] [batch][polys][L + 1][n] at chain_idx + 1 -> out[0] [batch][polys][E][n]          (RAW: in[0] raw words)
 *   TENSOR          in[0], in[1] [batch][2][E][n] -> out[0] [batch][3][E][n]
 *   TENSOR_CONV     in[0] [batch][sa][E][n], in[1] [batch][sb][E][n] -> out[0] [batch][sa + sb - 1][E][n]   (polys = sa, terms = sb)
 *   TENSOR_SUM      in[0], in[1] [batch][terms][2][E][n] -> out[0] [batch][terms][3][L][n] (e0 == 0 only), out[1] [batch][3][nBsk][n]
 *   BEHZ_FINISH     in[0] [batch][terms][3][E][n] -> out[0] [batch][3][L][n]   (ACCUMULATE: added to out[0]'s content; RAW: see below)
 *   BEHZ_FINISH_SUM in[0] [batch][terms][3][L][n], in[1] [batch][3][nBsk][n] -> out[0] [batch][3][L][n]     (RAW: see below)
 *   KS_INNER        in[0] [batch][L + 1][L][n], in[1] [K - 1][2][K][n] -> out[0] [batch][2][L + 1][n]
 *   KS_MODDOWN      in[0] [batch][2][L + 1][n] added into out[0] [batch][polys][L][n] (polys 2 or 3); n_ext > 0: out[1] [n_ext][2][E][n],
 *                   the BEHZ extension of the first n_ext results                                            (RAW: in[0] raw words)
 *   MODSWITCH, MODSWITCH_JOBS   in[0] [batch][polys][L][n] -> out[0] [batch][polys][L - 1][n]
 *   I0_FINISH       chain_idx = the level before the drop; in[0] [batch][2][L - 1][n], in[1] [batch][terms][2][n] -> out[0]
 *                   [batch][2][L - 1][n] (STORE: written, else added to its content)                  (RAW: in[0], in[1] raw words)
 *   EVAL_EPILOGUE   in[0] [batch][2][L][n], in[1] a0 [batch][n], in[2] mask [batch][n], in[3] / in[4] addends [batch][2][L][n] or
 *                   null, KEY: in[5] the RAW key-switch sums [batch][2][L + 1][n] -> out[0] [batch][2][n]
 *   ADD_MANY        in[0] [batch][terms][polys][L][n] added into out[0] [batch][polys][L][n];  SUM_JOBS: the same sums written
 *   ADD_PLAIN       in[0] [batch][n] mod t, scaled and added into out[0] [batch][L][n] (c0)
 *   DYADIC_PLAIN    in[0] [batch][polys][L][n], in[1] [batch][L][n] -> out[0] [batch][polys][L][n]
 *   LIFT            in[0] [batch][n] mod t, in[1] null or [batch] words (non-zero: not lifted) -> out[0] [batch][L][n]
 * RAW: the operand is what an inverse transform leaves when its limb's map entry carries the RAW mark -- any 64-bit word w, standing
 * for the residue w n^-1 psi^-k at coefficient k.  The finish of a level with L == nB <= 3 takes ONLY such input (flag required there,
 * refused elsewhere).  Every other operand is a canonical residue of its limb (or of plain_modulus).
 * Refusals, all APSU_HE_INVALID_ARGUMENT with the reason in apsu_he_last_error and nothing launched: an unknown step; a chain_idx that
 * is no data level; an array whose size is not the layout's; a word that is not canonical where the step needs a canonical one; RAW
 * where the launcher has no RAW form (DROP_BEHZ_EXT and the fused extension of KS_MODDOWN exist for L == nB <= 3 only, RAW KS_MODDOWN
 * and the KEY epilogue up to L = 4); a term count beyond the bound the engine checks on the host -- terms * q_widest < 2^63 for
 * BEHZ_FINISH_SUM, (terms + 1) * q_last < 2^64 for I0_FINISH.
 *
 * The kernels of a resident database, from POLYN_WITH_ROOTS on (same entry, same argument block, no new symbol; chain_idx is not
 * used).  They work modulo plain_modulus t on poly[rows][n], column s = the polynomial of bin (slot) s, coefficient d in row d.  Arrays of
 * 32-bit words and of bytes (counts, touched, tops, idx, flags, is_bin) travel as one 64-bit word per entry; 0xFFFFFFFF is LOOKUP_NONE,
 * a tile top of -1 is the word ~0.  "in/out": the array is copied up first, so a word the kernel does not write comes back as it went.
 *   POLYN_WITH_ROOTS polys = bins, terms = stride, e0 = max_deg; in[0] roots [bins][stride], in[1] counts [bins] -> out[0] poly [max_deg + 1][n]
 *   BINS_UPDATE      terms = rows, batch = bins, polys = ins_stride, e0 = rem_stride; in[0] touched [n_touched], in[1] ins [bins][ins_stride]
 *                    + in[2] ins_counts [bins] or both null, in[3] rem [bins][rem_stride] + in[4] rem_counts [bins] or both null;
 *                    out[0] poly [rows][n] in/out; out[1] counts_out [n_touched] in/out, then status[0] (lowest bin << 32 | position of a
 *                    removal that left a remainder, else ~0), status[1] (lowest touched bin that is the zero polynomial, else ~0)
 *   BIN_COUNTS       terms = rows; in[0] poly [rows][n] -> out[0] counts [n]
 *   POLY_DEGREE      terms = rows; in[0] poly [rows][n] -> out[0] one word
 *   BINS_LOOKUP      terms = degree; in[0] poly [degree + 1][n]; out[0] flags [parts] in/out.  polys = F, in[1] felts [count][F], in[2] start
 *                    [count]: the plan is lookup_plan's.  PLAN: in[1] work [n_work][4] (tile, row0, nrows, 0), in[2] pts [rows][64], in[3] idx
 *                    [rows][64] (a part or LOOKUP_NONE): the caller's own plan
 *   BINS_MERGE       terms = rows; in[0] A [rowsA][n], in[1] topsA [n / 64], in[2] B [rowsB][n], in[3] topsB [n / 64] -> out[0] C [rows][n]
 *   BINS_ROWS        terms = rows, polys = bins; in[0] poly [rows][n], in[1] counts [n] -> out[0] the ragged rows (off[bins] words or more)
 *                    in/out, out[1] off [bins + 1]
 *   BINS_EVAL        terms = rows; in[0] poly [rows][n], in[1] counts [n], in[2] x [n], in[3] mask [n] or null -> out[0] [n] in/out, out[1]
 *                    is_bin [n] in/out, then the bad flag (one word)
 *   EVAL_COMPARE     polys = count; in[0] got [count][n], in[1] want [count][n] -> out[0] mismatches, lowest (position << 32 | slot) or ~0
 *   ROOTS            terms = rows, e0 = hstride, batch = workgroups of the persistent search (0: the engine's number); COMPOSED: the
 *                    per-coset gather + transform + scan instead.  in[0] poly [rows][n]; the occupied bins are the columns whose highest
 *                    non-zero row is >= 1, in slot order -> out[0] hits [n_occ][hstride] in/out, out[1] found [n_occ], mult [n_occ][hstride]
 *                    in/out (written for the bins with fewer distinct roots than items only)
 *   UNLIFT           in[0] residues of q_0 as stored -> out[0] values mod t, as many words
 *   ROOTS_SPLIT      (numbered behind the transforms' steps) polys = k, e0 = hstride; in[0] hits [n_occ][hstride], in[1] found [n_occ],
 *                    in[2] mult [n_occ][hstride], in[3] counts [n]; the occupied bins are the slots with a count of 1 or more that is not
 *                    LOOKUP_NONE, in slot order; in[4] part_stride [k] -> out[0] the parts' root lists in/out, part p at the word
 *                    n * (part_stride[0] + .. + part_stride[p - 1]) as [n][part_stride[p]]; out[1] counts_out [k][n], then the failure
 *                    word (lowest slot << 32 | roots found with multiplicity of a bin that does not add up to its count, else ~0)
 * Refused like the others, nothing launched: rows of 0; a word >= t where the launcher's contract (device.h) wants a residue; a count
 * above its stride or, after the insertions, >= rows; a bin named twice in `touched`; a tile top outside -1 .. rows - 1; a work item or
 * index entry outside its plan; for ROOTS a degree >= n or a plain modulus with more than 65536 cosets; for UNLIFT a word that is
 * neither below t nor in q_0 - t .. q_0 - 1; for ROOTS_SPLIT k < 1, an hstride outside 1 .. 8192 or below a count, a value that
 * is read and is not below min(t, 2^32), a multiplicity that is read and exceeds 2^18, a part_stride below a bin's share of that part.
 *
 * The transforms, from NTT_INFO on (same entry, no new symbol; chain_idx is not used): launch_ntt, launch_ntt_gather and
 * launch_intt_tensor with the context's own tables and its own APSU_HE_NTT_LATENCY_LIMBS setting, so the choice of the launch form
 * and the split path at n = 32768 are part of what runs.  The caller gives the limb-to-modulus map the launcher reads: logical limb g
 * takes entry g % period, a modulus id (0 .. K-1 the key primes, K + i the i-th auxiliary prime, then plain_modulus where it
 * supports batching), plus APSU_HE_STEP_MAP_RAW in an inverse map: that limb comes back RAW (above).
 *   NTT_INFO        -> out[0]: log2 n, K, the number of auxiliary primes, batching (0 / 1), then the modulus of every modulus id
 *   NTT             in[0] [count][n] canonical, in[1] map [period]; INVERSE: the inverse transform -> out[0] [count][n]
 *   NTT_GATHER      in[0] sources [nsrc][n], in[1] the source of every output limb [count], in[2] map [period], in[3] max_src (one word,
 *                   NORED only) -> out[0] [count][n].  A source word is any 64-bit word; with NORED it is not reduced on load and must
 *                   be below max_src
 *   INTT_TENSOR     batch = njobs, terms = limbs, polys = stride (limbs between an operand's two polynomials, >= limbs; 0: limbs),
 *                   e0 = dgap (limbs between the outputs of two jobs, >= 3 limbs; 0: 3 limbs);
 *                   in[0] a [njobs][2][stride][n], in[1] b the same, both canonical, in[2] plain [n_plain][n] canonical or null, in[3] map
 *                   [period] over (job, polynomial of 3, limb) and then the plain limbs -> out[0] [njobs][dgap][n] in/out, job j's first
 *                   [3][limbs][n] = the inverse transforms of a0 b0, a0 b1 + a1 b0, a1 b1; out[1] [n_plain][n] the inverse transforms of the plain limbs
 * Refused like the others, nothing launched: a modulus id out of range; MAP_RAW in a forward map; NORED at n = 32768, with a target
 * for which max_src + 4 log2(n) q exceeds 2^64 or which is not narrow, or with a source word at or above max_src; a word that is not
 * canonical where canonical is asked; the three outputs of one operand limb under different moduli; INTT_TENSOR at n = 32768; sizes
 * that do not match (at most 4096 limbs per launch).
 *
 * The querier's side and the decryption, from SEED_EXPAND on (same entry, no new symbol): the launchers behind apsu_he_seed_expand,
 * apsu_he_keygen, apsu_he_relin_keygen, apsu_he_query_create and apsu_he_decrypt_decode, with the context's own level and key blocks
 * and its slot map.  `batch` is 1 .. 64.  A signed byte (the small polynomials) travels as one sign-extended 64-bit word.  out[0] is
 * in/out everywhere: a word the kernel does not write comes back as it went.
 *   SEED_EXPAND     chain_idx = the level (-1 or K - 1: the key level, L = K), terms = the list cap (1 .. 8192: the rejected positions an
 *                   object's list takes); in[0] seeds [batch][8], in[1] thresholds [L]: a word at or above its limb's threshold is
 *                   rejected (in place of SEAL's max_multiple) -> out[0] [batch][L][n]; out[1] [batch + 1]: every list's counter as the
 *                   fix-up pass left it (0 for a completed object, its number of rejected words for one that overflowed), then the
 *                   overflow word (1 when some object rejected more words than the cap; that object is incomplete, the others complete).
 *                   The lists are fresh for every call.
 *   DECRYPT_ROUND   in[0] ct [batch][2][n] (c0 is read, at stride 2 n), in[1] v [batch][n], in[2] q0, t (the launcher's arguments, need not
 *                   be the context's) -> out[0] [batch][n] = round(t (c0 + v mod q0) / q0) mod t.  ACCUMULATE: the launcher with the noise
 *                   budget's numerator, out[1] worst [batch] = max over the coefficients of min(r, q0 - r), r = t (c0 + v) mod q0
 *   PLAIN_POWERS    in[0] values [batch][n] (any words), in[1] exponents [S] (32 bits each, S = 1 .. 64) -> out[0] [batch * S][n]:
 *                   row b S + s holds values[b][i]^exponents[s] mod t at the slot BatchEncoder gives index i; a value >= t counts as 0
 *                   and raises bit 0 of the flag word out[1] [1]
 *   SAMPLE_SMALL    in[0] seed [8] -> out[0] [n] the secret's coefficients (batch 1, e0 0); KEY: out[0] [batch][n] the noise polynomials
 *                   of objects e0 .. e0 + batch - 1 (N5's stream layout, below)
 *   SMALL_LIFT      polys = limbs (1 .. K); in[0] small [batch][n] signed bytes -> out[0] [batch][limbs][n] residues of the key primes
 *   ENC_FINISH      chain_idx = the level; in[0] pt [batch][n] mod t, in[1] v [batch][L][n], in[2] e [batch][n] signed bytes; out[0] cts
 *                   [batch][2][L][n]: c0 = Delta(pt) - e - v per limb is written, the c1 halves are left alone
 *   RLK_FINISH      (batch 1) in[0] s [K][n], in[1] e [K - 1][K][n]; out[0] ksk [K - 1][2][K][n]: ksk[i][0][j] = -(ksk[i][1][j] s_j + e[i][j])
 *                   + [j == i] (p mod q_i) s_i^2 is written, the halves ksk[i][1] are read and left alone
 *   FLAG_MONOMIAL   in[0] pt [batch][n] (any words) -> out[0] [batch]: 1 where exactly one word is non-zero, else 0
 * Refused like the others, nothing launched: a list cap outside 1 .. 8192; a threshold below 2^62 (the fix-up redraws until a word
 * falls below its threshold: a small one would not end; every real one exceeds 2^63); for DECRYPT_ROUND t >= q0, q0 >= 2^62,
 * t >= 2^61, t < 2, a word of c0 or v that is not below q0; an exponent above 32 bits; PLAIN_POWERS without batching; a word that is
 * no sign-extended signed byte; a word of pt, v, s, e or an a half that is not canonical; RLK_FINISH in a context with one prime;
 * objects beyond the seed's range; sizes that do not match.
 *
 * The multiply-accumulate family, from MAC_INFO on (same entry, no new symbol): launch_mac, launch_term_product, launch_pack_rows,
 * launch_unpack_rows and launch_limb0_rows with the level block of chain_idx (L = chain_idx + 1 limbs).  A stored plaintext is a SLOT:
 * dense, [L][n] words; or bit-packed (flag PACKED): limb j is a row of n coefficients of w_j = mac_bits[j] bits, coefficient c in bits
 * [c w_j, (c + 1) w_j) of the little-endian bit string that starts at byte mac_row_off[j] of the slot, rows back to back, a slot of
 * n (w_0 + .. + w_{L-1}) / 8 bytes.  Bit-packed bytes travel as 64-bit words (little-endian; n is a multiple of 64, so a slot is whole
 * words).  Every bit-packed array a kernel READS is uploaded with 16 zero bytes behind it, as the engine keeps them.  out[0] is in/out
 * everywhere: a word the kernel does not write comes back as it went.  The geometry is read back from the device's level block.
 *   MAC_INFO        -> out[0] [2 + 7 L] = L, the bit-packed slot's bytes, then per limb mac_shift, mac_chunk, mac_chunk_k, mac_bits,
 *                   mac_row_off, mac_mask_hi, mac_kara_usable (0 / 1)
 *   MAC             ONE launch_mac over `batch` jobs (1 .. 64).  polys = streams per job (1 .. 4), terms = terms per chain (1 .. 4096),
 *                   e0 = limb0, n_ext = nl: a job multiplies limbs limb0 .. limb0 + nl - 1 and writes them as limbs 0 .. nl - 1.
 *                   Flags: KARA the three-product form, PACKED bit-packed plaintexts, LIMB_SLOW the grid order (block, job, limb)
 *                   instead of (block, limb, job); the grid is MacGrid{ mac_grid(n, batch).gx, LIMB_SLOW }, so either order runs
 *                   with a handful of jobs, and its limb extent is L as in the engine.
 *                   in[0] powers [batch][terms][2][P][n], P read from the size, L <= P <= 18 (pw_poly_stride = P n, pw_stride = 2 P n);
 *                   in[1] plaintexts [batch][polys][terms] slots (pt_stride = one slot); out[0] [batch][polys][2][n_ext][n]
 *                   (out_poly_stride = n_ext n): stream g of job b = sum over the terms of plaintext (.) power, per polynomial.
 *                   in[2] null, or a job table [batch][4] = limb0, nl, ng, cnt per job (nl <= n_ext, limb0 + nl <= L, 1 <= ng <= polys,
 *                   1 <= cnt <= terms): the job takes its first ng streams and cnt terms and leaves every other word of its part
 *                   of out[0] alone.  A stream the job does not have reads stream 0's plaintexts, as mac_plan sets it; its
 *                   output pointer is that stream's own part of out[0] (g < polys), where a store the kernel must not make shows,
 *                   and stream 0's beyond.
 *   TERM_PRODUCT    ONE launch_term_product on limb e0, dense or PACKED: `batch` operand sets (1 .. 64), each repeated `terms`
 *                   times -- job u < batch * terms (at most 2^17) reads set u % batch.  in[0] powers [batch][2][P][n], in[1]
 *                   plaintexts [batch] slots -> out[0] [batch * terms + 1][2][n]: job u writes its own [2][n]; the last [2][n]
 *                   is a guard behind the last job's output that no job owns.
 *   PACK_ROWS       batch = slots; in[0] dense [slots][L][n] -> out[0] the bit-packed slots, then two words (16 bytes) that no row owns
 *   UNPACK_ROWS     batch = slots; in[0] the bit-packed slots -> out[0] dense [slots][L][n]
 *   LIMB0_ROWS      batch = count (1 .. 65535); in[0] [count] slots, dense or PACKED -> out[0] [count][n], limb 0 of every slot
 *   ENTRIES_SCATTER (a database step, no chain level) ONE launch_entries_scatter for target BinBundle k = e0 of one bundle index:
 *                   batch = locations, polys = F, terms = stride; bits per field element, item_bit_count and cap = max_items_per_bin
 *                   - 1 are the context's.  in[0] items [count][2] words, count = offsets[batch] - offsets[0]; in[1] offsets [batch + 1];
 *                   in[2] kstart [batch], one word each -> out[0] roots [bins][stride], in/out (bins from its size, locations * F <=
 *                   bins <= n; the words nobody writes keep what they held), out[1] counts [n].  Refused: a chunk longer than stride,
 *                   offsets that decrease, F above 64 or (F - 1) * bits per field element >= 128, sizes that do not match.
 * Refused like the others, nothing launched: a chain_idx that is no data level; n no multiple of 64; PACKED in a context whose rows
 * are all 64 bits wide; for MAC polys outside 1 .. 4, terms 0 (or a cnt of 0), limb0 + nl beyond the level, P below L, KARA on a
 * level with a prime that mac_kara_usable rejects (59 and 60 bits), a job-table entry outside the ranges above; for MAC and
 * TERM_PRODUCT a word of the powers (limbs below L) or a coefficient of a plaintext -- a bit-packed one decoded on the host with
 * packed_coeff -- that is not a canonical residue of its limb; for TERM_PRODUCT a limb beyond the level; for PACK_ROWS a word that is
 * not canonical; for PACK_ROWS and UNPACK_ROWS slots * L above 65535, the y extent of their grid (the engine's own callers refuse the
 * same: pack_rows_grid_check, mac_plan.h); sizes that do not match.
 *
 * The grouping by location, from BUCKET_COUNT on (same entry, no new symbol; chain_idx is not used): the kernels behind
 * apsu_he_items_bucket_device one at a time, each through the launcher that the whole sort calls for it (launch_bucket.h), so grid and
 * block are the sort's.  A 32-bit array (locs, tile_cnt, hist, wave_cnt, order) travels one value per 64-bit word.  Every out[] is in/out:
 * a word the kernel does not write comes back as it went.  tile = keys (or items) per workgroup, a multiple of 256 in [256, 2^20];
 * waves = 4; D = 1 << width.
 *   BUCKET_COUNT    polys = H, terms = tile; in[0] locs [count][H] -> out[0] tile_cnt [key_tiles], key_tiles = ceil(count / tile): the entries
 *                   (i, h) of the tile's items with no g < h where locs[i][g] == locs[i][h]
 *   BUCKET_KEYS     the same geometry; in[1] the CALLER's tile_base [key_tiles] -> out[0] keys [room] (room from its size): tile t's keys
 *                   loc << 32 | i in (i, h) order from tile_base[t] on, no other word
 *   BUCKET_SCAN     in[0] [n] 32-bit values (null: n = 0) -> out[0] [n + 1]: out[k] = in[0] + .. + in[k - 1] for k < n, the last word a
 *                   guard.  STORE: out[1], one word, the sum of all; without the flag the launcher gets a null sum pointer, as in the
 *                   passes, and out[1] must be null
 *   BUCKET_HIST     terms = tile, e0 = shift, n_ext = width, batch = the tiles of the grid; in[0] keys [batch * tile], any 64-bit words;
 *                   in[1] total, one word -> out[0] hist [D][batch]: the keys of tile t below total with digit d = bits [shift, shift +
 *                   width) of the key; out[1] wave_cnt [batch][4][D]: the same over wave w's run, keys [w tile / 4, (w + 1) tile / 4) of the
 *                   tile cut at the tile's keys
 *   BUCKET_SCATTER  the same geometry; in[2] the CALLER's scanned [D][batch], in[3] the CALLER's wave_cnt [batch][4][D] -> out[0] [room]:
 *                   key -> place scanned[d][t] + wave_cnt[t][ww][d] over ww < w + its rank among the equal digits earlier in its
 *                   wave's run; no other word
 *   BUCKET_OFFSETS  terms = T; in[0] keys, ascending below total (null with a total of 0), in[1] total -> out[0] [T + 2]: offsets[l] =
 *                   the keys below total that are below l << 32, l <= T; the last word a guard
 *   BUCKET_ORDER    in[0], in[1] as for BUCKET_OFFSETS -> out[0] [room]: the low halves of the keys below total
 *   ENTRIES_GATHER  batch = room; in[0] items [count][2], in[1] order [room], in[2] total -> out[0] [room][2]: entry k = item order[k], k < total
 * Refused like the others, nothing launched: a tile size outside the rule; H outside 1 .. 8; count 0; T = 0; a width outside 1 .. 8; a
 * shift below 32 or shift + width above 64; a total above the keys given (or above the room); a 32-bit value that does not fit; for
 * BUCKET_KEYS a tile whose keys would reach beyond the room, for BUCKET_SCATTER a place at or beyond the room -- both worked out on the
 * host from the arrays given, so no step stores out of bounds; for BUCKET_OFFSETS keys below total that do not ascend; for
 * ENTRIES_GATHER an order word below total that names no item; sizes that do not match.
 *
 * The remaining launchers, from ADD on (same entry, no new symbol): the small kernels of the query path and the database-build path
 * that no step above reaches.  Every out[] is in/out; a guard is a word behind (or in front of) what the kernel owns.
 *   ADD             chain_idx = the level; in[0] x [batch][polys][L][n] added into out[0] acc [batch][polys][L][n] per limb (batch 1 .. 64,
 *                   polys 1 .. 8), both canonical
 *   CLEAR_BITS      e0 = bits (0 .. 63); out[0] [words + 1]: the low `bits` bits of the first `words` words are cleared, the last a guard
 *   COPY_JOBS       terms = words per job (even, >= 2), batch = jobs (1 .. 64); in[0] sources [jobs][words] -> out[0] [jobs][words + 2]:
 *                   job j's words, then two guard words
 *   COPY_SOURCES    chain_idx = the level, L = chain_idx + 1, words = 2 L n; batch = jobs; in[0] sources [jobs][2][L][n], or null: the
 *                   check in place, out[0] is source and destination; in[1] = the report word before the launch, seq (32 bits each)
 *                   -> out[0] [jobs][2][L][n]; out[1], one word: the report word after -- max(before, seq) when some word of some job
 *                   is at or above the prime of its limb, else as before
 *   FILL_RANDOM     in[0] = seed, bound (>= 1) -> out[0] [words + 1]: word i = splitmix64(seed + i) % bound (64-bit wrap), the last a guard
 *   FILL_BLAKE2XB   in[0] seed [8], in[1] = first, bound (>= 1) -> out[0] [1 + words + 1]: word 1 + i = the (first + i)-th 32-bit output of
 *                   SEAL's Blake2xb generator under the seed, % bound; a guard on both sides
 *   SCATTER_SLOTS   in[0] [batch][n], in[1] a permutation [n] or null: the context's slot map -> out[0] [batch][n]: out[b][map[i]] = in[b][i]
 *   GATHER_SLOTS    the same arguments: out[b][i] = in[b][map[i]]
 *   ALGEBRAIZE      polys = felts, terms = bits per felt, e0 = item_bit_count; in[0] items [count][2] (16 bytes, little-endian) -> out[0]
 *                   [count * felts + 1]: felt j = bits [j bpf, j bpf + bpf) of the item's first item_bit_count bits; the last a guard
 *   PACK_BLOCKS     polys = felts, terms = len (2 .. 63), e0 = items (items * felts <= n); in[0] values [batch][n] -> out[0] [batch][items][2]
 *                   + 1: (lower, higher) of the reference's vec_to_oc_block, the last word a guard
 * Refused like the others, nothing launched: a chain_idx that is no data level; a word of ADD's operands that is not canonical; bits
 * outside 0 .. 63; an odd word count for COPY_JOBS; a bound of 0; a map word >= n or a map that is no permutation, a null map in a
 * context without batching; felts outside 1 .. 64, bits per felt outside 1 .. 64, (felts - 1) * bits per felt >= 128, item_bit_count
 * outside 1 .. 128; len outside 2 .. 63; items * felts above n; batch outside 1 .. 64; sizes that do not match. */
enum { APSU_HE_STEP_LEVEL_INFO = 0, APSU_HE_STEP_BEHZ_EXT, APSU_HE_STEP_DROP_BEHZ_EXT, APSU_HE_STEP_TENSOR, APSU_HE_STEP_TENSOR_CONV,
       APSU_HE_STEP_TENSOR_SUM, APSU_HE_STEP_BEHZ_FINISH, APSU_HE_STEP_BEHZ_FINISH_SUM, APSU_HE_STEP_KS_INNER, APSU_HE_STEP_KS_MODDOWN,
       APSU_HE_STEP_MODSWITCH, APSU_HE_STEP_MODSWITCH_JOBS, APSU_HE_STEP_I0_FINISH, APSU_HE_STEP_EVAL_EPILOGUE, APSU_HE_STEP_ADD_MANY,
       APSU_HE_STEP_SUM_JOBS, APSU_HE_STEP_ADD_PLAIN, APSU_HE_STEP_DYADIC_PLAIN, APSU_HE_STEP_LIFT,
       APSU_HE_STEP_POLYN_WITH_ROOTS, APSU_HE_STEP_BINS_UPDATE, APSU_HE_STEP_BIN_COUNTS, APSU_HE_STEP_POLY_DEGREE, APSU_HE_STEP_BINS_LOOKUP,
       APSU_HE_STEP_BINS_MERGE, APSU_HE_STEP_BINS_ROWS, APSU_HE_STEP_BINS_EVAL, APSU_HE_STEP_EVAL_COMPARE, APSU_HE_STEP_ROOTS, APSU_HE_STEP_UNLIFT,
       APSU_HE_STEP_NTT_INFO, APSU_HE_STEP_NTT, APSU_HE_STEP_NTT_GATHER, APSU_HE_STEP_INTT_TENSOR,
       APSU_HE_STEP_ROOTS_SPLIT,
       APSU_HE_STEP_SEED_EXPAND, APSU_HE_STEP_DECRYPT_ROUND, APSU_HE_STEP_PLAIN_POWERS, APSU_HE_STEP_SAMPLE_SMALL, APSU_HE_STEP_SMALL_LIFT,
       APSU_HE_STEP_ENC_FINISH, APSU_HE_STEP_RLK_FINISH, APSU_HE_STEP_FLAG_MONOMIAL,
       APSU_HE_STEP_MAC_INFO, APSU_HE_STEP_MAC, APSU_HE_STEP_TERM_PRODUCT, APSU_HE_STEP_PACK_ROWS, APSU_HE_STEP_UNPACK_ROWS,
       APSU_HE_STEP_LIMB0_ROWS,
       APSU_HE_STEP_ENTRIES_SCATTER,
       APSU_HE_STEP_BUCKET_COUNT, APSU_HE_STEP_BUCKET_KEYS, APSU_HE_STEP_BUCKET_SCAN, APSU_HE_STEP_BUCKET_HIST, APSU_HE_STEP_BUCKET_SCATTER,
       APSU_HE_STEP_BUCKET_OFFSETS, APSU_HE_STEP_BUCKET_ORDER, APSU_HE_STEP_ENTRIES_GATHER,
       APSU_HE_STEP_ADD, APSU_HE_STEP_CLEAR_BITS, APSU_HE_STEP_COPY_JOBS, APSU_HE_STEP_COPY_SOURCES, APSU_HE_STEP_FILL_RANDOM,
       APSU_HE_STEP_FILL_BLAKE2XB, APSU_HE_STEP_SCATTER_SLOTS, APSU_HE_STEP_GATHER_SLOTS, APSU_HE_STEP_ALGEBRAIZE, APSU_HE_STEP_PACK_BLOCKS };
enum { APSU_HE_STEP_RAW = 1, APSU_HE_STEP_ACCUMULATE = 2, APSU_HE_STEP_STORE = 4, APSU_HE_STEP_KEY = 8, APSU_HE_STEP_PLAN = 16,
       APSU_HE_STEP_COMPOSED = 32, APSU_HE_STEP_INVERSE = 64, APSU_HE_STEP_NORED = 128, APSU_HE_STEP_KARA = 256, APSU_HE_STEP_PACKED = 512,
       APSU_HE_STEP_LIMB_SLOW = 1024 };
#define APSU_HE_STEP_MAP_RAW ((uint64_t)1 << 30)   /* in a map entry of an inverse transform */
typedef struct {
    int32_t step, chain_idx;
    uint32_t flags;
    int32_t terms, polys, batch, e0, n_ext;
    const uint64_t *in[6];
    size_t in_words[6];
    uint64_t *out[2];
    size_t out_words[2];
} apsu_he_step_args;
int apsu_he_debug_run_step(apsu_he_ctx *ctx, const apsu_he_step_args *args);
/* N1, compaction: the way back from many sparse BinBundles to few full ones.  The placement rule tries BinBundles newest first and
 * drops one only when it is empty, so after insertions and removals a bundle index keeps several half-empty BinBundles, and each costs
 * every query its fixed share: the high-power ciphertext products, a key switch, one result ciphertext, one block of PEQT / OT work.
 * The union of two bins is the PRODUCT of their polynomials, so BinBundles are merged without anybody's roots: each input is decoded to
 * its bins' polynomials mod plain_modulus (as by the update), the polynomials of equal slots are multiplied (k_bins_merge: lane = slot,
 * a wave holds 8 output coefficients of 64 slots in registers; products are summed unreduced, in one 64-bit word for a plain modulus
 * below 2^32 and in 128 bits above, and reduced once per fold interval), and the tail of the build re-encodes.
 * apsu_he_bundles_merge: n_bundles >= 2 BinBundles of ONE bundle index -> *out, a NEW BinBundle with that bundle index and the given
 * cache_idx, holding per bin the union of the inputs' bins.
 *  - The list of a bin is a multiset: a value that two inputs hold in the same bin is a double root of the merged bin, and one
 *    removal (apsu_he_bundle_update) takes out one occurrence.
 *  - If the inputs are build_bundle(B_1) .. build_bundle(B_k), the image of the result (apsu_he_bundle_save) is byte-identical to that
 *    of build_bundle of the bin-wise union, in whatever order the inputs are given.  Degree, level, Paterson-Stockmeyer layout,
 *    monomial flags and row packing follow from the merged counts as in the build.
 *  - A merged BinBundle answers apsu_he_bundles_lookup, apsu_he_bundle_update and queries like any other.  The false-positive note of
 *    apsu_he_bundles_lookup applies to fuller bins as it does to the reference's: every part present in its bin, each from another item.
 *  - A slot that holds the zero polynomial in every input keeps it.  Refused (APSU_HE_INVALID_ARGUMENT, apsu_he_last_error names the
 *    first slot, no bundle is produced): a bin whose summed count reaches max_items_per_bin -- the placement rule's strict bound, so no
 *    merged bin exceeds max_items_per_bin - 1; inputs whose sets of bins differ (a slot that is a bin in one and holds the zero
 *    polynomial in another); inputs of different bundle indices; fewer than two inputs.
 *  - The inputs are only read and stay valid until the caller frees them (queued evaluations may still read them).
 * apsu_he_db_compact: for the BinBundles of ONE bundle index, given in cache order as for apsu_he_db_apply_entries:
 * apsu_he_bundle_bin_counts of each, then the rule -- walk them in cache order; a BinBundle joins the FIRST earlier group that has the
 * same set of bins and, for every bin, count_group + count_bundle < max_items_per_bin (strictly), else it opens a new group; a group's
 * counts grow as BinBundles join -- then one apsu_he_bundles_merge per group of two or more.
 *  - group[i], i < n_bundles: the group of BinBundle i; groups are numbered 0, 1, .. in the order of their first members.
 *  - merged[g]: the NEW BinBundle of group g, with the cache_idx of the group's first member; NULL for a group of one, whose BinBundle
 *    stays as it is, and for g at or above the number of groups (merged has n_bundles entries, all written).  *n_merged (may be NULL):
 *    the number of handles produced.  The caller replaces the members of a merged group by merged[g] and frees them when no queued
 *    evaluation reads them any more.  A second call on the result merges nothing.
 * Preconditions and locking are the update's (PSUParams, batching, first coefficient prime above 2 * plain_modulus; synchronous;
 * apsu_he_db_compact takes the context's lock per step).  The multi-device handle has its own forms, apsu_he_multi_db_merge_bundles
 * and apsu_he_multi_db_compact. */
int apsu_he_bundles_merge(apsu_he_ctx *ctx, const apsu_he_bundle *const *bundles, uint32_t n_bundles, uint32_t cache_idx,
                          apsu_he_bundle **out);
int apsu_he_db_compact(apsu_he_ctx *ctx, uint32_t bundle_idx, const apsu_he_bundle *const *bundles, uint32_t n_bundles, uint32_t *group,
                       apsu_he_bundle **merged, uint32_t *n_merged);
/* N1, splitting and moving: the two maintenance steps that the calls above lacked.  Neither takes a root to the host.
 * apsu_he_bundle_split: ONE BinBundle -> `parts` NEW BinBundles out[0 .. parts), the inverse of apsu_he_bundles_merge.  A bin holds the
 * sorted multiset r_0 <= .. <= r_{c-1}; with cut(p) = floor(p c / parts), part p holds the positions [cut(p), cut(p + 1)) of it.
 *  - Every part of every bin therefore has floor(c / parts) or ceil(c / parts) items; equal values may straddle a cut (the parts are
 *    multisets); an empty bin is empty (the polynomial 1) in every part; a slot that is not a bin is not a bin in any part.
 *  - Every part keeps the input's bundle index and takes cache_idx[p]; cache_idx NULL: the input's own for part 0 and the numbers
 *    behind it.
 *  - How: apsu_he_bundle_bins' decode, counts and root search; then k_roots_split, one workgroup per occupied bin, sorts the bin's
 *    distinct roots (64-bit keys value << 32 | multiplicity in LDS, a bitonic network), scans the multiplicities and writes every
 *    part's items to a list of that part on the device; then the tail of the build per part.  The host decides every part's counts
 *    and degree from the input's counts alone.
 *  - If b is build_bundle(B), any update or merge of such, or such a BinBundle loaded from an image, the image of part p
 *    (apsu_he_bundle_save) is byte-identical to that of build_bundle of part p of B, and apsu_he_bundles_merge of the parts has b's image.
 *  - Refused (APSU_HE_INVALID_ARGUMENT, apsu_he_last_error names the slot where there is one, no BinBundle is produced): parts < 1;
 *    parts above the largest bin count when that count is 1 or more; bins that are not a prefix of the slots (the build makes
 *    prefixes only); a bin whose polynomial does not split into linear factors (the first such slot, its count, the roots found,
 *    as by apsu_he_bundle_bins).  APSU_HE_LOGIC_ERROR as there: a plain modulus with more than 65536 cosets, a degree >= n.
 *  - The number of parts that brings every bin below a bound `limit` is the smallest k with ceil(largest count / k) < limit; with
 *    limit = max_items_per_bin the parts take insertions and can be exported (apsu_he_bundle_export_saved refuses a bin at the bound).
 * apsu_he_bundle_adopt, called on the DESTINATION context with the source context and one of ITS BinBundles -> *out, a NEW BinBundle
 * of dst with the same bins, bundle index b's, cache index as given.  The two parameter sets must agree in poly_modulus_degree,
 * plain_modulus, felts_per_item, table_size and hash_func_count (so every item lies in the same bin of the same bundle index);
 * coeff_modulus_bits, ps_low_degree, query_powers and max_items_per_bin are free.  Between two such contexts a stored plaintext is
 * the same polynomial mod plain_modulus, so the coefficient half of the source's decode and the destination's own build tail move
 * it: no slot transform, no root search.
 *  - The image in dst is byte-identical to dst's build_bundle of the same bins: level, Paterson-Stockmeyer layout, monomial flags
 *    and the row format of dst's own APSU_HE_PACKED_ROWS.
 *  - Refused (APSU_HE_INVALID_ARGUMENT): parameters that differ in one of the five fields (the message names the first); a degree
 *    above dst's max_items_per_bin (the message says into how many parts to split first); contexts on different devices.
 *    APSU_HE_LOGIC_ERROR: a source whose first coefficient prime is not above 2 * plain_modulus.
 *  - The contexts' locks are taken one after the other, never both.
 * apsu_he_db_rebase: the BinBundles of one call, from src to dst: apsu_he_bundle_bin_counts of each, then per BinBundle either
 * apsu_he_bundle_adopt, or -- where its largest bin does not stay below dst's max_items_per_bin -- apsu_he_bundle_split in src into the
 * smallest number of parts that does, apsu_he_bundle_adopt of each part and release of the parts.
 *  - out[i], i < *n_out: the NEW BinBundles of dst in input order, the parts of one input consecutive; origin[i]: the position in
 *    `bundles` it came from; cache_idx[i] (may be NULL): dense per bundle index, by position.  `capacity`: the room in out / origin /
 *    cache_idx; *n_out is written even when it is too small (which is refused).
 *  - All or nothing: on any refusal every BinBundle made so far is released and no handle is produced.
 *  - It does not compact: where dst allows fuller bins, apsu_he_db_compact there does.
 * Preconditions and locking otherwise are the update's.  The multi-device handle has no forms of these yet. */
int apsu_he_bundle_split(apsu_he_ctx *ctx, const apsu_he_bundle *b, uint32_t parts, const uint32_t *cache_idx, apsu_he_bundle **out);
int apsu_he_bundle_adopt(apsu_he_ctx *dst, apsu_he_ctx *src, const apsu_he_bundle *b, uint32_t cache_idx, apsu_he_bundle **out);
int apsu_he_db_rebase(apsu_he_ctx *dst, apsu_he_ctx *src, const apsu_he_bundle *const *bundles, uint32_t n_bundles, apsu_he_bundle **out,
                      uint32_t *origin, uint32_t *cache_idx, uint32_t capacity, uint32_t *n_out);
/* device time of the context's last apsu_he_bundle_split: decode and counts, root search and multiplicities, k_roots_split, the builds */
int apsu_he_debug_split_times(apsu_he_ctx *ctx, double *decode_ms, double *roots_ms, double *split_ms, double *build_ms);
/* device time of the context's last apsu_he_bundles_merge: the decodes and counts, the product kernels, the re-encode */
int apsu_he_debug_merge_times(apsu_he_ctx *ctx, double *decode_ms, double *kernel_ms, double *encode_ms);
/* "next" row N2: engine-native image of one BinBundle cache (256-byte header with a parameter
 * fingerprint and checksum + the raw limb arrays), the GPU-resident counterpart of ReceiverDB::save / Load
 * (receiver/apsu/receiver_db.cpp:1182-1429, bin_bundle.fbs).  The buffer may be an mmap of a file. */
int apsu_he_bundle_image_size(apsu_he_ctx *ctx, const apsu_he_bundle *b, uint64_t *bytes);
int apsu_he_bundle_save(apsu_he_ctx *ctx, const apsu_he_bundle *b, uint8_t *buf, uint64_t capacity, uint64_t *written);
int apsu_he_bundle_load(apsu_he_ctx *ctx, const uint8_t *buf, uint64_t size, apsu_he_bundle **out);
/* "next" row N4: the per-BinBundle host work either side of the evaluation, on the GPU.
 * apsu_he_mask_generate replaces the "random gen" block of Receiver::RunQuery (receiver/apsu/receiver_osn.cpp:217-284):
 * for each of `count` BinBundles, n slot values uniform mod plain_modulus, BatchEncoder::encode of them
 * (masks_dev: count*n words on the device, the `masks` of apsu_he_eval_bundles with masks_on_device = 1), and
 * vec_to_oc_block of every item (receiver_osn.cpp:53-73; blocks: count*items_per_bundle*2 words, (low, high)
 * halves of the 128-bit block; host; may be NULL).  values (host, count*n; may be NULL) receives the slot values.
 * The reference draws them from SEAL's Blake2xb PRNG under a fresh random seed; here value(c, i) =
 * splitmix64(seed + (c*n + i + 1) * 0x9e3779b97f4a7c15) mod plain_modulus — a different uniform stream, the
 * same encode and packing.
 * apsu_he_decrypt_decode is the querier's side of a loopback check (sender/apsu/sender_osn.cpp:675-700,
 * common/apsu/network/result_package.cpp:175-213): Decryptor::decrypt of `count` results (size 2, last level,
 * 2*n words each), BatchEncoder::decode, and the same block packing.  sk_ntt: the secret key modulo q_0 in NTT
 * form (n words, host).  The rounding is the exact round(t*x/q_0): equal to SEAL's decrypt for every
 * ciphertext with a positive noise budget. */
int apsu_he_mask_generate(apsu_he_ctx *ctx, uint64_t seed, uint32_t count, uint64_t *masks_dev, uint64_t *values, uint64_t *blocks);
/* The same with the reference's own generator (receiver_osn.cpp:221-224: UniformRandomGeneratorInfo(prng_type::blake2xb,
 * seed).make_prng(); :248-251: `generate() % plain_modulus`, generate() being SEAL's 32-bit draw): seed = the eight words of
 * seal::prng_seed_type (the reference fills them with random_bytes); value(c, i) = (output number first_value + c*n + i of that
 * generator) % plain_modulus, so one call with first_value = 0 over the BinBundles in the reference's loop order
 * (cache_idx outer, bundle_idx inner, padded caches skipped) reproduces its masks for the same seed, and several calls
 * can continue one stream.  BLAKE2b is checked against RFC 7693 / hashlib; the BLAKE2X expansion and SEAL's buffering
 * (4096-byte buffers keyed by the seed, message = buffer counter) are restated from their published sources — unpinned,
 * like every other SEAL-derived detail. */
int apsu_he_mask_generate_blake2xb(apsu_he_ctx *ctx, const uint64_t seed[8], uint64_t first_value, uint32_t count, uint64_t *masks_dev,
                                   uint64_t *values, uint64_t *blocks);
int apsu_he_decrypt_decode(apsu_he_ctx *ctx, const uint64_t *sk_ntt, const uint64_t *cts, int cts_on_device, uint32_t count,
                           uint64_t *values, uint64_t *blocks);
/* ---- N5 (added after ABI 7, additive): the querier's side of the HE path -- APSU's *sender*  -----------------------
 * apsu_he_keygen + apsu_he_relin_keygen replace Sender::reset_keys (sender/apsu/sender_osn.cpp:215-229: KeyGenerator, secret key,
 * create_relin_keys); apsu_he_query_create replaces the prepare_data / encrypt_data blocks of Sender::create_query (:426-484:
 * PlaintextPowers, BatchEncoder::encode, Encryptor::encrypt_symmetric; plaintext_powers.cpp:41-46,51-99);
 * apsu_he_decrypt_decode_budget is apsu_he_decrypt_decode with the invariant noise budget ResultPackage::extract also reports
 * (common/apsu/network/result_package.cpp:175-213).  The OPRF stays with the caller; the cuckoo table and its slot values are
 * apsu_he_cuckoo_table's and apsu_he_query_values' (below).
 *
 * Randomness.  SEAL draws through std::uniform_int_distribution and its bootstrap generator, which no restatement can pin; the
 * streams here are the engine's own.  Every draw of a call is a function of u[0], u[1], ...: the 32-bit outputs of SEAL's Blake2xb
 * generator (blake2x.h; the generator of apsu_he_mask_generate_blake2xb) under the caller's 64-byte seed[8].  A 64-bit draw at an
 * even position p is w = u[p] + 2^32 u[p + 1].  With B = 16 outputs per 64-byte stream block:
 *   secret s             coefficient k:  w at p = 2k                                        (blocks [0, 4096))
 *                        s_k = floor(3 w / 2^64) - 1, uniform over {-1, 0, 1} up to 2^-64
 *   public seed          of object o:    the 16 outputs u[B (4096 + o)], ... as eight 64-bit words   (blocks [4096, 4096 + 2^20))
 *   noise e of object o  coefficient k:  w at p = B (2^21 + 4096 o) + 2k                    (blocks 2^21 + 4096 o + [0, 4096))
 *                        e_k = popcount(bits 0..20 of w) - popcount(bits 21..41 of w): SEAL's centred binomial, |e| <= 21, variance 10.5
 * Objects: o = i for relinearisation key i (i < 16); o = 16 + c for ciphertext c of apsu_he_query_create.  One noise polynomial per
 * object, shared by its limbs.  The ranges are disjoint for every poly_modulus_degree <= 32768 and o < 2^20 (apsu_amd/csrc/query_side.h
 * holds the constants).  The public seeds are outputs of the secret stream; nothing secret is drawn from a public seed.
 * The seed is key material and must come from the operating system's generator.  The three calls of one querier may share a seed
 * (their ranges are disjoint); two queries must not -- a second apsu_he_query_create needs a fresh seed.
 *
 * apsu_he_keygen: sk_ntt[K][n] = s modulo every key prime, NTT form; sk_ntt[0] is what apsu_he_decrypt_decode takes.
 * apsu_he_relin_keygen: key i = (-(a_i s + e_i) + [limb == i] (p mod q_i) s^2, a_i) over the K limbs in NTT form, p = the special
 * prime, a_i = the expansion of its public seed at the key level as apsu_he_seed_expand(chain_idx = -1) gives it.  ksk (host,
 * [K-1][2][K][n], the layout of apsu_he_relin_upload), key_seeds (host, [K-1][8], what apsu_he_seal_relin_keys_save takes) and out (the
 * keys resident on the device, no host round trip) may each be NULL.  A parameter set without key switching: APSU_HE_INVALID_ARGUMENT.
 * apsu_he_query_create: values[b][n] (host, or device with values_on_device) = the slot values (algebraized items, < plain_modulus) of
 * bundle index bundle_indices[b].  cts_dev (DEVICE memory, n_bundle_idx * source_power_count * 2 * L * n words, L = first_chain_idx + 1):
 * ciphertext b * source_power_count + s = encryption of BatchEncoder::encode(x^e mod t per slot), e = the s-th source power (ascending);
 * size 2, coefficient form, first data level -- the order apsu_he_compute_powers(src_on_device = 1) reads.  ct_seeds (host, [count][8]):
 * the public seed of every c1, so that apsu_he_seal_ct_save(seed) writes the seeded object: c1 = apsu_he_seal_sample_poly_uniform(seed),
 * c0 = Delta(m) - e - c1 s with the scaling of apsu_he_add_plain.  Every word is a canonical residue.  At most 65535 ciphertexts per call.
 * A value >= plain_modulus, a secret-key word >= its prime, a bundle index out of range: APSU_HE_INVALID_ARGUMENT.  Synchronous.
 * apsu_he_decrypt_decode_budget: budget_bits[count] = Decryptor::invariant_noise_budget of each result,
 * floor(log2(q_0 / (2 max_k |t x_k mod q_0|))) with x the phase c0 + c1 s (the bit count of q_0 for a noiseless result). */
int apsu_he_keygen(apsu_he_ctx *ctx, const uint64_t seed[8], uint64_t *sk_ntt);
int apsu_he_relin_keygen(apsu_he_ctx *ctx, const uint64_t *sk_ntt, const uint64_t seed[8], uint64_t *ksk, uint64_t *key_seeds, apsu_he_relin **out);
int apsu_he_query_create(apsu_he_ctx *ctx, const uint64_t *sk_ntt, const uint64_t seed[8], const uint32_t *bundle_indices, int n_bundle_idx,
                         const uint64_t *values, int values_on_device, uint64_t *cts_dev, uint64_t *ct_seeds);
int apsu_he_decrypt_decode_budget(apsu_he_ctx *ctx, const uint64_t *sk_ntt, const uint64_t *cts, int cts_on_device, uint32_t count,
                                  uint64_t *values, uint64_t *blocks, int32_t *budget_bits);
/* N1, one step earlier: util::algebraize_item (common/apsu/util/db_encoding.cpp:209-256,360-366; called at
 * receiver_db.cpp:296-298 on every OPRF'd item) for `count` hashed items of 16 bytes each: felts[i * felts_per_item + j] =
 * bits [j*b, (j+1)*b) of item i's first item_bit_count bits, read as a little-endian bit string, b = bit_count(plain_modulus) - 1.
 * These are the roots apsu_he_db_build_bundle takes once the host has placed them into bins.  (ABI 4) */
int apsu_he_algebraize_items(apsu_he_ctx *ctx, const uint8_t *items, size_t count, int items_on_device, uint64_t *felts, int felts_on_device);
/* N1, cuckoo hashing for both parties (added after ABI 7, additive): where an item goes (receiver_db.cpp:57-79,262-300) and the
 * querier's table (sender_osn.cpp:329-460), without Kuku.  Both parties must agree on the location function bit for bit.
 *
 * Kuku 2.x LocFunc [Kuku-recall]: restated from memory and UNPINNED, like the SEAL object layer -- no Kuku source and no known-answer
 * vector has been held against it.  item_type is 16 bytes, location_type uint32_t.  The seed of function f is make_item(f, 0): f as 8
 * little-endian bytes, then 8 zero bytes.  tab_f[16][256] (uint32) = the 16384 bytes of blake2xb(out = 16384, in = the 16 seed bytes,
 * no key) read as little-endian words: root hash under the parameter block {digest 64, key 0, fanout 1, depth 1, xof_length 16384},
 * then 256 expansion nodes {digest 64, key 0, fanout 0, depth 0, leaf_length 64, node_offset i, xof_length 16384, node_depth 0,
 * inner_length 64} over the root.  loc_f(item) = (tab_f[0][item[0]] ^ tab_f[1][item[1]] ^ ... ^ tab_f[15][item[15]]) % table_size for
 * f < hash_func_count, both from the context's PSUParams (a context without them: APSU_HE_LOGIC_ERROR).
 *
 * apsu_he_item_locations: locs[count][hash_func_count] of items[count][16]; each a host pointer, or a device pointer with its flag.
 * apsu_he_items_bucket (the database side): the locations on the device, then a stable counting sort by location on the host.
 *   offsets[table_size + 1], order[count * hash_func_count] (host; *total = offsets[table_size] words of order are written): bucket l =
 *   order[offsets[l] .. offsets[l + 1]) lists the items that have l among their locations, in input order; an item whose functions
 *   collide on l appears once (the unordered_set of all_locations).  That is oprf_in of receiver_db.cpp:264-289 flattened, hence the
 *   order in which the reference emits entries.  Every listed item is one ENTRY of apsu_he_db_apply_entries: its (OPRF'd) item through
 *   apsu_he_algebraize_items, bundle index l / items_per_bundle, start bin (l % items_per_bundle) * felts_per_item.  The buckets of
 *   one bundle index are contiguous in order: offsets[b * items_per_bundle] .. offsets[(b + 1) * items_per_bundle].
 * apsu_he_items_bucket_device (added after ABI 7, additive): the same offsets and order with the grouping on the device too, and the
 *   entries gathered there.  apsu_he_items_bucket stays as it is: the second implementation of the same contract.
 *   - offsets[table_size + 1]: host, always.  order (may be NULL): count * hash_func_count words of room, host or, with order_on_device,
 *     device memory; *total = offsets[table_size] words are written, the words behind them are not.  entries (may be NULL):
 *     [count * hash_func_count][16] of room, host or, with entries_on_device, device memory of any alignment; entries[k] =
 *     items[order[k]] for k < *total, which is exactly what apsu_he_db_build_from_entries reads (after the caller's OPRF).
 *   - The output is the sequence of the surviving pairs (location, item) in ascending (location, item) order, a pure function of
 *     the input: the words are the same on every run.  Method: keys location << 32 | item of the surviving entries, compacted in
 *     input order by a prefix sum; a stable least-significant-digit radix sort on the ceil(log2 table_size) bits of the location, in
 *     digits of at most 8 bits (two passes for every shipped parameter file), each pass a histogram per tile, one exclusive scan over
 *     (digit, tile) and a stable scatter whose ranks come from ballots within a wave and counts across waves -- never from the return
 *     value of an atomic; offsets by bisection of the sorted keys; one 16-byte load and store per gathered entry (k_entries_gather).
 *     No workgroup waits for another: every pass over the data is a launch of its own on the context's stream.
 *   - count = 0: offsets all zero, *total = 0, nothing is launched.  count >= 2^32 - 1: APSU_HE_INVALID_ARGUMENT.  Synchronous.
 * apsu_he_debug_bucket_locs (test hook, any context): the grouping alone on caller-given locs[count][hash_func_count] (host) for a
 *   caller-given function count (1 .. 8) and table size (>= 1), offsets and order on the host.  tile_entries: the keys per tile of the
 *   passes, a multiple of 256 from 256 to 2^20, or 0 for the engine's choice (8192); the result does not depend on it.  Anything else,
 *   and a location >= table_size (the message names its index): APSU_HE_INVALID_ARGUMENT, nothing written.
 * apsu_he_debug_bucket_times: device time of the context's last apsu_he_items_bucket_device: the locations, the grouping (keys, passes,
 *   offsets and order), the gather.
 *
 * apsu_he_cuckoo_table (the querier's side).  The reference inserts sequentially with a random walk under its own generator; the
 * protocol needs only that every item sits at one of its own locations, so the table is built by the engine's own deterministic,
 * order-independent rule.  Item i starts with function index h_i = 0 and is active.  Rounds r = 0 .. max_rounds - 1 (the reference's
 * cuckoo_table_insert_attempts is 500; max_rounds outside [1, 2^32], the round's share of the key: APSU_HE_INVALID_ARGUMENT):
 *   propose  every active item takes the 64-bit minimum on slot[loc_{h_i}(i)] with the key ((max_rounds - 1 - r) << 32) | i.  An empty
 *            slot holds ~0, so a newer round beats any older occupant and within a round the lowest index wins.
 *   settle   (after a barrier) every item that is not a duplicate reads its slot.  Its own key: it is placed.  Otherwise, the winner's
 *            16 bytes equal its own: it is a DUPLICATE of the winner for good (the lowest index of equal items survives; the
 *            reference's "skipping repeated insertion").  Otherwise h_i = (h_i + 1) % hash_func_count and it is active again.
 *   The build is done when no item is active.  An item still active after max_rounds: APSU_HE_RUNTIME_ERROR, the message names the
 *   lowest such item and the fill rate, and nothing is written.
 *   table_idx[table_size]: the item of each slot or 0xFFFFFFFF; item_loc[count]: the location of each item, 0xFFFFFFFF for a duplicate;
 *   *rounds (may be NULL): rounds run.  Outputs are host memory.  One workgroup (k_cuckoo_insert); the slots live in LDS up to 8184 of
 *   them and in the context's workspace beyond, with the same result.  With uniformly random locations (NOT Kuku's, which nobody has
 *   measured) every shipped (set size, table_size) pair with three functions finished within 37 rounds over 60 seeds each, fill <= 0.676.
 * apsu_he_query_values: table_items[table_size][16] = the table after the caller's OPRF (the caller fills the slots from table_idx;
 *   an empty slot holds what the caller's protocol puts there, { 0, 0 } in the reference) -> values[bundle_idx_count][n]: slot
 *   b * items_per_bundle + k, algebraized as by apsu_he_algebraize_items, fills positions k * felts_per_item .. + felts_per_item - 1 of
 *   row b; positions from bins_per_bundle to n are 0 (sender_osn.cpp:433-460 and BatchEncoder's padding).  Exactly what
 *   apsu_he_query_create(values_on_device) reads.
 * apsu_he_debug_item_locations / apsu_he_debug_cuckoo_insert: test hooks on host arrays -- the location kernel with a caller-given
 *   function count and table size; the table rule on caller-given items[count][16] and locs[count][hash_func_count] (the tests steer
 *   collisions no item set can steer).  form: 0 the engine's choice, 1 LDS (a table that does not fit: APSU_HE_LOGIC_ERROR), 2 workspace.
 * All are synchronous and serialised on the context like every other call. */
int apsu_he_item_locations(apsu_he_ctx *ctx, const uint8_t *items, size_t count, int items_on_device, uint32_t *locs, int locs_on_device);
int apsu_he_items_bucket(apsu_he_ctx *ctx, const uint8_t *items, size_t count, int items_on_device, uint64_t *offsets, uint32_t *order,
                         uint64_t *total);
int apsu_he_items_bucket_device(apsu_he_ctx *ctx, const uint8_t *items, size_t count, int items_on_device,
                                uint64_t *offsets,                       /* host, table_size + 1 */
                                uint32_t *order, int order_on_device,    /* count * hash_func_count words of room; may be NULL */
                                uint8_t *entries, int entries_on_device, /* [count * hash_func_count][16] of room; may be NULL */
                                uint64_t *total);
int apsu_he_debug_bucket_locs(apsu_he_ctx *ctx, const uint32_t *locs, size_t count, uint32_t hash_func_count, uint32_t table_size,
                              uint32_t tile_entries,                     /* 0: the engine's choice */
                              uint64_t *offsets, uint32_t *order, uint64_t *total);   /* host arrays */
int apsu_he_debug_bucket_times(apsu_he_ctx *ctx, double *locs_ms, double *sort_ms, double *gather_ms);
int apsu_he_cuckoo_table(apsu_he_ctx *ctx, const uint8_t *items, size_t count, int items_on_device, uint64_t max_rounds, uint32_t *table_idx,
                         uint32_t *item_loc, uint64_t *rounds);
int apsu_he_query_values(apsu_he_ctx *ctx, const uint8_t *table_items, int table_items_on_device, uint64_t *values, int values_on_device);
int apsu_he_debug_item_locations(apsu_he_ctx *ctx, const uint8_t *items, size_t count, uint32_t hash_func_count, uint32_t table_size,
                                 uint32_t *locs);
int apsu_he_debug_cuckoo_insert(apsu_he_ctx *ctx, const uint8_t *items, const uint32_t *locs, size_t count, uint32_t hash_func_count,
                                uint32_t table_size, uint64_t max_rounds, int form, uint32_t *table_idx, uint32_t *item_loc, uint64_t *rounds);
/* N1, checking a resident database against plaintext (added after ABI 7, additive).  The image checksum protects bytes, not meaning:
 * a BinBundle whose stored limbs do not describe one plaintext, one encoded under another ps_low_degree, one merged from a damaged
 * input, or one held under parameters whose noise budget is too small passes it, and the first sign is a wrong union at the end of
 * the protocol.  These two calls say, on the device, what a resident BinBundle should answer to a query and whether the engine's own
 * homomorphic path answers that.
 * apsu_he_bundles_eval_plain: out[b][s] = P_{b,s}(x[b][s]) + masks[b][s] mod plain_modulus, P_{b,s} the polynomial BinBundle b holds in
 * slot s -- the value the querier who sent x[b] decrypts in that slot, and what decrypt(eval(query)) is checked against.
 *  - x[n_bundles][n], n = poly_modulus_degree: slot values below plain_modulus; the caller repeats a bundle index's query for each of
 *    its BinBundles.  masks[n_bundles][n]: slot values (what apsu_he_mask_generate* return in `values`), NOT the encoded plaintexts
 *    that apsu_he_eval_bundles takes; NULL: no masks.  out[n_bundles][n].  Each is a host pointer, or a device pointer with its flag set.
 *  - is_bin (may be NULL): [n_bundles][n] bytes on out's side, 1 where the slot is a bin, 0 where it holds the zero polynomial.  Such a
 *    slot yields masks[b][s] alone, as the homomorphic path does.  A member of a bin (a root of its polynomial) yields the mask alone too.
 *  - The BinBundles are decoded and evaluated one after the other through the context's workspace, as by apsu_he_bundles_lookup
 *    (k_bins_eval: one Horner walk per slot with lane = slot, every stored coefficient read once, a tile of 64 slots walking from its
 *    own largest count).  They are only read.
 *  - A value >= plain_modulus, in x or masks, on the host or the device: APSU_HE_INVALID_ARGUMENT (a device-side value is found by
 *    the kernel; out is then written but means nothing).
 * Preconditions and locking are apsu_he_bundle_bin_counts's.  Synchronous.  Parameter sets without key switching are served.
 * apsu_he_debug_eval_plain_times: device time of the context's last such call, summed over its BinBundles: decode, counts, k_bins_eval.
 *
 * apsu_he_db_self_test: one call that runs the whole loop on the device for `count` BinBundles of this context and compares.  In order:
 * apsu_he_keygen; apsu_he_relin_keygen; apsu_he_query_create for the distinct bundle indices among `bundles`; apsu_he_compute_powers
 * with device sources; apsu_he_mask_generate_blake2xb; apsu_he_eval_bundles with masks on the device; apsu_he_decrypt_decode_budget;
 * apsu_he_bundles_eval_plain on the same slot and mask values; a comparison kernel, slot for slot.
 *  - x (may be NULL): [distinct bundle indices, ascending][n] slot values below plain_modulus (host).  NULL: drawn mod plain_modulus
 *    from the Blake2xb stream of `seed` like the masks, as 32-bit outputs u[p]: the i-th distinct bundle index takes
 *    p = 2^37 + i n + [0, n) (stream blocks from 2^33), the mask of the BinBundle at position b takes p = 2^38 + b n + [0, n) (blocks
 *    from 2^34).  The querier's ranges (above, apsu_amd/csrc/query_side.h) end below block 2^33, so one seed serves the whole call.
 *    A drawn x is almost never an item of the database; pass items to have the test cover members (they decrypt to the mask alone).
 *  - report: BinBundles and slots checked; mismatches; the first mismatch in (position in `bundles`, slot) order with the value
 *    decrypted and the value expected, first_bundle = -1 for none; the smallest noise budget over the results and the first BinBundle
 *    that has it; device time of the homomorphic part (key generation to decryption) and of the plain part (evaluation and comparison).
 *  - APSU_HE_OK whenever the test ran: mismatches are a result, not an error.  A noise budget of 0 bits shows as mismatches too.
 *  - The secret key and the relinearisation keys never leave device buffers of the call; those buffers, and the context's workspace
 *    through which the key generation passed them, are overwritten with zeros before they are released, whichever way the call ends.
 *    The seed is key material all the same.
 *  - A parameter set without key switching: APSU_HE_INVALID_ARGUMENT, as from apsu_he_relin_keygen (apsu_he_bundles_eval_plain serves
 *    those).  Other preconditions as above.  At most 2^20 - 1 BinBundles.  Synchronous; the context's lock is taken per step.
 * What a clean report proves: the engine's own evaluation, its decryption and the stored polynomials agree with each other for these
 * parameters -- upload, layout, Paterson-Stockmeyer split, key switching, noise.  What it cannot prove: agreement with SEAL.  Both
 * sides are this engine's restatement of the reference; that stays unpinned.  Nor that the polynomials are the
 * intended ones: a stored plaintext that is wrong but well-formed (another a_0, say) reads the same on both sides -- another database.
 * apsu_he_debug_self_test_times: device time in ms of the context's last self-test: decode, counts, k_bins_eval (each summed over the
 * BinBundles), the comparison, the homomorphic part.
 * apsu_he_multi_db_self_test (declared with the handle's calls below): every device tests the BinBundles it owns, devices side by side,
 * under the handle's lock; every device creates the query for the bundle indices of the whole handle and draws BinBundle id's mask at
 * position id, so the draws are those of one context holding the BinBundles in id order.  The reports are reduced: counts summed, the
 * first mismatch and the smallest budget named by BinBundle id (lowest id first), the times of the slowest device. */
typedef struct {
    uint32_t bundles, reserved;
    uint64_t slots, mismatches;
    int32_t first_bundle;            /* position in `bundles` (multi-device handle: BinBundle id); -1: no mismatch */
    uint32_t first_slot;
    uint64_t first_got, first_expected;
    int32_t min_budget_bits, min_budget_bundle;   /* -1: nothing was checked */
    double he_ms, plain_ms;
} apsu_he_self_test_report;
int apsu_he_bundles_eval_plain(apsu_he_ctx *ctx, const apsu_he_bundle *const *bundles, uint32_t n_bundles, const uint64_t *x, int x_on_device,
                               const uint64_t *masks, int masks_on_device, uint64_t *out, int out_on_device, uint8_t *is_bin);
int apsu_he_debug_eval_plain_times(apsu_he_ctx *ctx, double *decode_ms, double *counts_ms, double *kernel_ms);
int apsu_he_db_self_test(apsu_he_ctx *ctx, const apsu_he_bundle *const *bundles, uint32_t count, const uint64_t seed[8], const uint64_t *x,
                         apsu_he_self_test_report *report);
int apsu_he_debug_self_test_times(apsu_he_ctx *ctx, double *ms5);
/* N2 for the whole database -- the counterpart of ReceiverDB::save / Load (receiver/apsu/receiver_db.cpp:1182-1429) for a DB
 * that lives in HBM as raw limb arrays: ONE file per parameter set = header with the parameter fingerprint, a table
 * (bundle index, cache index, degree, offset, size) and the BinBundle images above at 4096-byte aligned offsets.  The file is
 * mapped (mmap), so a process touches only the BinBundles it loads, each array going to the device with one copy from the
 * mapping: a device of a node reads its shard of a 75 GiB database, not the file.  apsu_he_db_file_save writes to path + ".tmp"
 * and renames.  A file written for other parameters, truncated or with a damaged table / image is refused
 * (APSU_HE_INVALID_ARGUMENT).  (ABI 4) */
typedef struct apsu_he_db_file apsu_he_db_file;
int apsu_he_db_file_save(apsu_he_ctx *ctx, const char *path, const apsu_he_bundle *const *bundles, int count);
int apsu_he_db_file_open(const char *path, apsu_he_db_file **out);
int apsu_he_db_file_close(apsu_he_db_file *f);
int apsu_he_db_file_count(const apsu_he_db_file *f, int *count, uint64_t *file_bytes);
int apsu_he_db_file_entry(const apsu_he_db_file *f, int i, uint32_t *bundle_idx, uint32_t *cache_idx, uint32_t *degree, uint64_t *image_bytes);
int apsu_he_db_file_load(apsu_he_ctx *ctx, const apsu_he_db_file *f, int i, apsu_he_bundle **out);
/* test hooks: degree of the batched polynomial; stored form of coefficient `degree`
 * (kind 0: raw mod t [n]; 1: NTT form [(plain_level+1)*n]; 2: pre-lifted + NTT at the high level [(high+1)*n]) */
int apsu_he_bundle_degree(const apsu_he_bundle *b, uint32_t *degree);
int apsu_he_bundle_download(apsu_he_ctx *ctx, const apsu_he_bundle *b, uint32_t degree, uint64_t *out, size_t capacity_words,
                            size_t *words, int *kind);
/* Polynomials of a target power after ComputePowers and of one BinBundle's result: 2 with key switching.  Without it
 * (one coefficient prime) the reference never relinearises: a product has size(parent1) + size(parent2) - 1 polynomials,
 * eval's result the size of its longest power, eval_patstock's the size of its longest product (at least 3). */
int apsu_he_power_size(const apsu_he_ctx *ctx, uint32_t power, uint32_t *polys);
int apsu_he_bundle_result_size(const apsu_he_ctx *ctx, const apsu_he_bundle *b, uint32_t *polys);
int apsu_he_bundle_free(apsu_he_bundle *b);
int apsu_he_bundle_bytes(const apsu_he_bundle *b, uint64_t *db_bytes);
/* Receiver::ComputePowers for n_bundle_idx bundle indices at once (receiver_osn.cpp:320-328,395-488).
 * src_cts[b * source_power_count + s] = query ciphertext of the s-th source power (ascending) for
 * bundle index bundle_indices[b]: size 2, coefficient form, first data level (receiver_osn.cpp:304-317).
 * src_on_device != 0: the pointers are device pointers (inputs already resident in HBM).
 * Every coefficient must be a canonical residue of its limb's prime, which is what a valid seal::Ciphertext holds
 * (seal::is_data_valid_for, checked by SEALObject::extract in the reference, seal_object.h:161-219): the engine's lazy transforms
 * take source limbs as they are.  apsu_he_run_query_request checks it on the decoded objects and fails like the reference; device-resident
 * sources are checked by the kernel that gathers them, and a violation is reported (APSU_HE_INVALID_ARGUMENT) by the call that next
 * waits for that work: a synchronous apsu_he_eval_bundles, apsu_he_powers_download or apsu_he_sync. */
int apsu_he_compute_powers(apsu_he_ctx *ctx, const uint32_t *bundle_indices, int n_bundle_idx,
                           const uint64_t *const *src_cts, int src_on_device, const apsu_he_relin *rk,
                           apsu_he_powers **out);
int apsu_he_powers_free(apsu_he_powers *p);
/* test hook: copy one computed power back (form/level per receiver_osn.cpp:459-487); words = apsu_he_power_size * (level+1) * n */
int apsu_he_powers_download(apsu_he_ctx *ctx, const apsu_he_powers *p, uint32_t bundle_idx, uint32_t power,
                            uint64_t *out, size_t capacity_words, int *chain_idx, int *is_ntt);
/* Receiver::ProcessBinBundleCache -> BatchedPlaintextPolyn::eval / eval_patstock for `count`
 * BinBundles (receiver_osn.cpp:490-540 ; bin_bundle.cpp:106-174,192-360).  masks[i] = random_plain
 * (n coefficients mod t, receiver_osn.cpp:217-284).  out_cts: count * 2 * n words, result i at
 * out_cts + i*2*n, last level, irrelevant bits cleared.  *_on_device: pointers are device pointers.
 * Parameter sets without key switching: rows of apsu_he_info.result_polys * n words, result i = its first
 * apsu_he_bundle_result_size polynomials, zeros behind them. */
int apsu_he_eval_bundles(apsu_he_ctx *ctx, const apsu_he_bundle *const *bundles, int count, const apsu_he_powers *powers,
                         const apsu_he_relin *rk, const uint64_t *const *masks, int masks_on_device, uint64_t *out_cts,
                         int out_on_device);

/* ---- several GPUs of one node behind one handle ------------------------------------------------------------------
 * The in-process counterpart of Receiver::RunQuery's fan-out (receiver/apsu/receiver_osn.cpp:320-364: ComputePowers per
 * bundle index, then one ProcessBinBundleCache task per BinBundle on the thread pool).  One engine and one host thread per
 * device; the BinBundle is the sharded unit: devices are assigned to bundle indices first (a device then needs the
 * powers of few indices only), an index's BinBundles are split over its devices by cost ~ degree.  A query's only data
 * exchange is the final gather of the fixed-size results.  Devices may repeat (e.g. {0, 0}) to rehearse
 * the multi-device path on one GPU.  (bench.py's one-process-per-GPU launch uses the same partition rule and RCCL.) */
typedef struct apsu_he_multi apsu_he_multi;
/* the partition rule alone (no GPU needed): device slot of each BinBundle (bundle_idx, cache_idx, degree) */
int apsu_he_partition_bundles(uint32_t bundle_idx_count, int n_devices, const uint32_t *bundle_idx, const uint32_t *cache_idx,
                              const uint32_t *degree, int count, int *device_slot);
/* The same with a spill pass: compute_powers_cost = what ComputePowers for ONE bundle index costs in the rule's unit (degree + 64
 * per BinBundle; apsu_he_compute_powers_cost gives the MI355X figure for a context's PowersDag).  BinBundles then move off the
 * slowest device to devices of OTHER bundle indices while that lowers the slowest device's cost including the second
 * ComputePowers the receiving device has to run (3 bundle indices on 8 devices: one index has two devices and 1.5x the load). */
int apsu_he_partition_bundles_ex(uint32_t bundle_idx_count, int n_devices, const uint32_t *bundle_idx, const uint32_t *cache_idx,
                                 const uint32_t *degree, int count, uint64_t compute_powers_cost, int *device_slot);
int apsu_he_compute_powers_cost(const apsu_he_ctx *ctx, uint64_t *cost);
int apsu_he_multi_create(const char *psu_params_json, const int *devices, int n_devices, apsu_he_multi **out);
int apsu_he_multi_destroy(apsu_he_multi *m);
int apsu_he_multi_device_count(const apsu_he_multi *m, int *n_devices);
/* polynomials per output row of apsu_he_eval_all(_ex) = apsu_he_info.result_polys of the parameter set (2 with key switching) */
int apsu_he_multi_result_polys(const apsu_he_multi *m, uint32_t *polys);
/* the query's RelinKeys, replicated on every device (layout as apsu_he_relin_upload) */
int apsu_he_multi_relin_upload(apsu_he_multi *m, const uint64_t *ksk);
/* DB placement (ReceiverDB::generate_caches, receiver_db.cpp:808-820): as apsu_he_db_upload_bundle / _random_bundle on the
 * device in `device_slot` (take it from apsu_he_partition_bundles).  *bundle_id = registration order = the BinBundle's
 * row in apsu_he_eval_all's masks and output. */
int apsu_he_multi_db_upload_bundle(apsu_he_multi *m, int device_slot, uint32_t bundle_idx, uint32_t cache_idx, uint32_t n_coeffs,
                                   const uint64_t *const *coeff_ptrs, const uint8_t *is_ntt, int *bundle_id);
int apsu_he_multi_db_random_bundle(apsu_he_multi *m, int device_slot, uint32_t bundle_idx, uint32_t cache_idx, uint32_t degree,
                                   uint64_t seed, int *bundle_id);
/* the whole file onto the handle's devices: BinBundles placed by apsu_he_partition_bundles_ex's rule (spill pass included), every
 * device reading its own shard from the shared mapping, all devices at once; bundle ids = the file's table order (appended to
 * what is registered already).  apsu_he_multi_db_save_file writes every registered BinBundle, in id order, into one file. */
int apsu_he_multi_db_load_file(apsu_he_multi *m, const apsu_he_db_file *f, int *n_loaded);
int apsu_he_multi_db_save_file(apsu_he_multi *m, const char *path);
int apsu_he_multi_db_clear(apsu_he_multi *m);
/* apsu_he_bundle_update on BinBundle `bundle_id` of the handle (see there) */
int apsu_he_multi_db_update_bundle(apsu_he_multi *m, int bundle_id, const uint64_t *ins_roots, const uint32_t *ins_counts,
                                   uint32_t ins_stride, const uint64_t *rem_roots, const uint32_t *rem_counts, uint32_t rem_stride,
                                   uint32_t bins);
/* ---- the resident database maintained on the handle: file -> load -> insert / remove items -> compact -> query, for a database
 * that lies on several devices.  The kernels and the host steps are the single context's (apsu_he_bundle_bin_counts, apsu_he_bundles_lookup,
 * apsu_he_db_apply_entries, apsu_he_bundles_merge, apsu_he_db_compact: their contracts hold here); every BinBundle is worked on by the
 * device that owns it, devices work side by side.  Added without an ABI step (additive; the ABI stays 7).  What a handle adds:
 *  - IDS STAY DENSE.  A BinBundle's id is its row in apsu_he_eval_all's masks and output.  A handle that never calls the functions
 *    below numbers by registration order, as before.  A call that drops BinBundles renumbers: survivors keep their relative order and
 *    take 0, 1, ..; BinBundles appended by the call follow in order of appending; a merged BinBundle takes the place of its group's
 *    first member in cache order.  new_id[old id] is the id from now on, -1 for a dropped BinBundle; the caller moves its masks and
 *    reads its result rows accordingly.  new_id may be NULL.
 *  - PLACEMENT.  A new BinBundle goes to the least loaded device (load = sum of degree + 64, the partition rule's unit) among those
 *    the partition rule's first pass gives its bundle index: the slots r with r % bundle_idx_count == bundle_idx when the handle has at
 *    least as many devices as bundle indices, else the slot bundle_idx % devices; ties go to the lowest slot.  The spill pass is not
 *    re-run; apsu_he_multi_db_move_bundle rebalances by hand.  A merged BinBundle is made on the device of its group's first member in
 *    cache order; members on other devices travel there device to device (no host image).
 *  - ALL OR NOTHING.  New BinBundles are built first; ids and rows change only when every step on every device has succeeded, and
 *    after the owning engines have finished what was queued on the old rows.  After a refusal the handle answers exactly as before.
 *  - Every call takes the handle's lock (ordered against apsu_he_eval_all and each other) and is synchronous.
 *  - CACHE ORDER of a bundle index: ascending cache_idx.  Two BinBundles of one bundle index with the same cache_idx make
 *    apsu_he_multi_db_index_bundles, _lookup, _apply_entries and _compact refuse with APSU_HE_INVALID_ARGUMENT.
 * apsu_he_multi_db_bundle_info: where BinBundle `bundle_id` lies and what it is (every output may be NULL).
 * apsu_he_multi_db_index_bundles: the ids of one bundle index in cache order; *n = how many there are, the first min(*n, capacity) are written.
 * apsu_he_multi_db_bin_counts: apsu_he_bundle_bin_counts on the owning device.
 * apsu_he_multi_db_bundle_bins: apsu_he_bundle_bins on the owning device, under the handle's lock.
 * apsu_he_multi_db_self_test: apsu_he_db_self_test of every device's BinBundles, see there; positions in the report are BinBundle ids.
 *   Run on a device list that repeats one GPU; two distinct GPUs have not run it.
 * apsu_he_multi_db_build_bundle: apsu_he_db_build_bundle on device_slot, or with device_slot = -1 on the slot the placement rule
 *   chooses; the new BinBundle is registered last (*bundle_id = the count before the call).
 * apsu_he_multi_db_remove_bundle: drops one BinBundle; new_id[count before the call].
 * apsu_he_multi_db_move_bundle: the BinBundle's arrays go to device_slot, device to device; it keeps its id, and its image
 *   (apsu_he_bundle_save) is the same bytes.  A move to the slot it is on does nothing.
 * apsu_he_multi_db_lookup: apsu_he_bundles_lookup against the BinBundles of apsu_he_multi_db_index_bundles(bundle_idx), rows in that order.
 * apsu_he_multi_db_apply_entries: apsu_he_db_apply_entries on the BinBundles of apsu_he_multi_db_index_bundles(bundle_idx).  Targets
 *   are OLD ids: the id a BinBundle had before the call, and (count before the call) + k for the k-th appended BinBundle; new_id
 *   [count before the call + *n_appended, at most + n_ins] translates them.  EMPTY BinBundles are dropped by the call itself.  Appended
 *   BinBundles are placed one after the other, against the loads as the call's updates left them (an EMPTY BinBundle still counts).
 * apsu_he_multi_db_build_from_entries: apsu_he_db_build_from_entries on the handle (host entries only).  The plan is computed once on
 *   the host; BinBundle (bundle index b, k) is built on the slot the placement rule gives it, in (b, k) order, the loads taken as each one
 *   registers; ids are appended densely: *first_id = the count before the call, *n_built the plan's total.  Refused if the handle
 *   already holds a BinBundle of a bundle index that receives entries (that case is apsu_he_multi_db_apply_entries').  All or nothing.
 * apsu_he_multi_db_merge_bundles: apsu_he_bundles_merge on n_ids >= 2 BinBundles of one bundle index, wherever they lie.  The merged
 *   BinBundle takes the id slot and the cache_idx of the first member in cache order; the others are dropped.  new_id[count before the call].
 * apsu_he_multi_db_compact: apsu_he_db_compact's rule on apsu_he_multi_db_index_bundles(bundle_idx), one merge per group of two or more;
 *   *n_merged (may be NULL) = merged BinBundles made.  new_id[count before the call].  A second call merges nothing. */
int apsu_he_multi_db_bundle_count(apsu_he_multi *m, int *count);
int apsu_he_multi_db_bundle_info(apsu_he_multi *m, int bundle_id, int *device_slot, uint32_t *bundle_idx, uint32_t *cache_idx, uint32_t *degree);
int apsu_he_multi_db_index_bundles(apsu_he_multi *m, uint32_t bundle_idx, int *ids, int capacity, int *n);
int apsu_he_multi_db_bin_counts(apsu_he_multi *m, int bundle_id, uint32_t *counts);
int apsu_he_multi_db_bundle_bins(apsu_he_multi *m, int bundle_id, uint64_t *roots, uint32_t *counts, uint32_t stride);
int apsu_he_multi_db_self_test(apsu_he_multi *m, const uint64_t seed[8], apsu_he_self_test_report *report);
int apsu_he_multi_db_build_bundle(apsu_he_multi *m, int device_slot, uint32_t bundle_idx, uint32_t cache_idx, const uint64_t *roots,
                                  const uint32_t *counts, uint32_t bins, uint32_t stride, int *bundle_id);
int apsu_he_multi_db_remove_bundle(apsu_he_multi *m, int bundle_id, int *new_id);
int apsu_he_multi_db_move_bundle(apsu_he_multi *m, int bundle_id, int device_slot);
int apsu_he_multi_db_lookup(apsu_he_multi *m, uint32_t bundle_idx, const uint64_t *felts, const uint32_t *start_bins, size_t count,
                            uint8_t *present, uint32_t *room);
int apsu_he_multi_db_apply_entries(apsu_he_multi *m, uint32_t bundle_idx, const uint64_t *ins_felts, const uint32_t *ins_start, size_t n_ins,
                                   const uint64_t *rem_felts, const uint32_t *rem_start, size_t n_rem, int *new_id, uint32_t *n_appended,
                                   uint32_t *ins_status, uint32_t *ins_target, uint32_t *rem_status, uint32_t *rem_target);
int apsu_he_multi_db_build_from_entries(apsu_he_multi *m, const uint8_t *entries, const uint64_t *offsets, int *first_id, uint32_t *n_built);
int apsu_he_multi_db_merge_bundles(apsu_he_multi *m, const int *bundle_ids, uint32_t n_ids, int *new_id);
int apsu_he_multi_db_compact(apsu_he_multi *m, uint32_t bundle_idx, int *new_id, uint32_t *n_merged);
/* One query on all devices (receiver_osn.cpp:304-364): src_cts[b * source_power_count + s] = host ciphertext of source
 * power s (ascending) of bundle index b, for EVERY bundle index (each device uploads the ones it needs); masks[id] = n
 * words mod t (host).  out_cts: bundle count * 2n words, row = bundle id; host memory when out_device_slot < 0, else
 * device memory on that device (rows gathered with peer copies over xGMI). */
int apsu_he_eval_all(apsu_he_multi *m, const uint64_t *const *src_cts, const uint64_t *const *masks, uint64_t *out_cts,
                     int out_device_slot);
/* The same with the caller saying where its buffers live (flags) -- the query arrives from the network into host memory
 * (receiver_osn.cpp:290-317), a co-located producer may already hold it in HBM:
 *   APSU_HE_IO_SRC_PINNED / _MASKS_PINNED / _OUT_PINNED  that host buffer is page-locked AND device-visible (apsu_he_host_alloc,
 *       hipHostMalloc): the kernels that consume / produce it anyway (ComputePowers' source gather, the evaluation's epilogue)
 *       read and write it in place over PCIe -- no copy at all.  Unflagged host buffers are pageable and go through each
 *       device's own page-locked area (a few helper threads do the staging copy).
 *   APSU_HE_IO_SRC_ON_DEVICE / _MASKS_ON_DEVICE  the pointers are device pointers on devices[in_device_slot]; every device with
 *       peer access reads them in place over xGMI (the others get copy-engine peer copies).
 *   APSU_HE_IO_GATHER_RCCL  (out_device_slot >= 0) the gather is ONE RCCL all-gather of fixed-size rows (ncclAllGather over
 *       xGMI; librccl.so is loaded on first use) instead of the default, in which every device's epilogue kernel stores its
 *       rows straight into the output device's buffer (peer writes; copy-engine peer copies without peer access).  Falls back
 *       to the default when RCCL is absent or the device list repeats a device (apsu_he_multi_last_gather: "rccl" / "peer").
 * Nothing of a device's share is waited for before its last kernel is queued. */
#define APSU_HE_IO_SRC_PINNED 1u
#define APSU_HE_IO_MASKS_PINNED 2u
#define APSU_HE_IO_OUT_PINNED 4u
#define APSU_HE_IO_SRC_ON_DEVICE 8u
#define APSU_HE_IO_MASKS_ON_DEVICE 16u
#define APSU_HE_IO_GATHER_RCCL 32u
int apsu_he_eval_all_ex(apsu_he_multi *m, const uint64_t *const *src_cts, const uint64_t *const *masks, uint64_t *out_cts,
                        int out_device_slot, unsigned flags, int in_device_slot);
const char *apsu_he_multi_last_gather(const apsu_he_multi *m);
/* page-locked host memory for query buffers (any thread, any device) */
int apsu_he_host_alloc(size_t bytes, void **out);
int apsu_he_host_free(void *p);
/* phase timers of the multi-device entry (see apsu_he_phase_*): arrays of APSU_HE_PHASES; "Receiver::RunQuery" is the HOST
 * wall time of apsu_he_eval_all(_ex) (uploads and downloads included), the other two the slowest device's device time */
int apsu_he_multi_phase_enable(apsu_he_multi *m, int on);
int apsu_he_multi_phase_read(apsu_he_multi *m, uint64_t *count, double *avg_ms, double *min_ms, double *max_ms, int reset);

/* Scheduling option: ComputePowers may walk the high-power half of the PowersDag on a second HIP stream, next to the
 * low-power half and to the BinBundle inner products (bit-identical results).  mode -1 = default policy (on
 * whenever the PowersDag splits into independent halves and the inputs are device resident), 0 = off, 1 = on; the environment variable APSU_HE_SPLIT=0/1
 * (read at apsu_he_create) sets the default for contexts that never call this.  Event profiling (apsu_he_profile_enable) always uses one stream. */
int apsu_he_set_two_stream(apsu_he_ctx *ctx, int mode);

/* Device-resident pipelines: with on != 0, an apsu_he_eval_bundles call whose masks AND results live in device memory
 * returns as soon as its work is queued (apsu_he_compute_powers with device-resident sources always does).  The results
 * are complete after apsu_he_sync(ctx), or for work ordered after the context's main HIP stream (apsu_he_stream: a
 * hipStream_t; e.g. hipEventRecord on it + hipStreamWaitEvent on the consumer's stream).  The caller's device buffers must
 * stay alive and unmodified until then.  Host-memory arguments always synchronise, as does event profiling.
 * Default off. */
int apsu_he_set_async_results(apsu_he_ctx *ctx, int on);
/* Overlap of consecutive queries (ABI 6; modes 2 and 3 ABI 7).  With mode != 0 the caller promises that the device-resident inputs
 * of apsu_he_compute_powers -- the source ciphertexts and the relinearisation keys -- are COMPLETE when the call is made, i.e. not
 * still being produced by work queued on the context's stream (apsu_he_stream).  The engine's second stream then does not wait for
 * the main stream's queue at the start of a ComputePowers (receiver_osn.cpp:395-488) but only for the last evaluation that read the
 * powers buffer it is about to reuse, and a ComputePowers that finds an evaluation still running on the device is queued as ONE
 * chain on the second stream next to it (pipelined queries: -4 % on the rate of queued queries; one query alone takes the same
 * time).  mode 0 (default): off -- a caller that uploads a query on the context's stream and calls apsu_he_compute_powers behind it
 * (apsu_he_run_query_request does) needs the ordering.  1: on.  2: on, without the pipelined walk (only the high-power chain starts
 * early).  3: on, every ComputePowers takes the pipelined walk whether or not the device is busy (for tests: the walk's event chain
 * is exercised deterministically; slower for a query that runs alone).  Results are bit-identical in every mode. */
int apsu_he_set_query_overlap(apsu_he_ctx *ctx, int mode);
/* Tier 1 on device-resident operands (ABI 5): with on != 0 every pointer argument of the tier-1 calls (apsu_he_transform_to_ntt ...
 * apsu_he_clear_irrelevant_bits; relinearisation keys stay handles) is DEVICE memory -- or page-locked host memory, which the device
 * addresses -- and the calls return with their work queued on the context's stream instead of copying in, waiting and copying out:
 * a caller that replaces Evaluator methods one by one (receiver_osn.cpp:422-478, bin_bundle.cpp:143-170) keeps its ciphertexts in
 * HBM across calls and pays no host round trip per method.  Ordering and completion as for apsu_he_set_async_results:
 * calls on one context execute in call order; apsu_he_sync / apsu_he_stream give the completion point.  Default off.
 * Precondition: host operands of the tier-1 calls are checked like seal::is_data_valid_for (every word of limb j below q_j, else
 * APSU_HE_INVALID_ARGUMENT); device operands are NOT read back for that check -- every word the caller hands over must already be a
 * canonical residue of its limb's prime, or the result is undefined (the kernels take canonical input). */
int apsu_he_set_tier1_on_device(apsu_he_ctx *ctx, int on);
int apsu_he_sync(apsu_he_ctx *ctx);
int apsu_he_stream(apsu_he_ctx *ctx, void **hip_stream);

/* ---- "next" row N3: the network framing around the path, without flatc / flatbuffers / SEAL -----------------
 * What the reference pins is the FlatBuffers framing of its messages; these functions read and write it:
 *   ReceiverOperationHeader                   common/apsu/network/rop_header.fbs ; receiver_operation.cpp:27-87
 *   ReceiverOperation{QueryRequest}           common/apsu/network/rop.fbs        ; receiver_operation.cpp:180-350
 *   ReceiverOperationResponse{QueryResponse}  common/apsu/network/rop_response.fbs
 *   ResultPackage                             common/apsu/network/result_package.fbs ; result_package.cpp:29-150
 * All buffers are size-prefixed (FinishSizePrefixed), exactly what ZMQChannel / StreamChannel carry.  The byte vectors
 * inside (Ciphertext.data, QueryRequest.relin_keys) are SEAL's own serialisation (seal_object.h:161-219); the reference
 * does not pin that format, so they are passed through as opaque byte ranges.  Parsers verify every offset, length and
 * alignment before use (like flatbuffers::Verifier) and fail with the reference's messages; returned pointers point INTO
 * the caller's buffer.  Builders return a malloc'ed buffer to release with apsu_he_wire_buffer_free.
 * ReceiverOperationType: 0 unknown, 1 parms, 2 oprf, 3 query, 4 response. */
typedef struct apsu_he_wire_query apsu_he_wire_query;
int apsu_he_wire_buffer_free(uint8_t *p);
int apsu_he_wire_build_header(uint32_t version, uint32_t type, uint8_t **out, size_t *out_size);
int apsu_he_wire_parse_header(const uint8_t *buf, size_t size, uint32_t *version, uint32_t *type);
/* ReceiverOperationQuery::save (receiver_operation.cpp:180-247): part i holds cts_per_part[i] ciphertext blobs, taken in
 * order from ct_data / ct_sizes; relin_keys NULL = field absent. */
int apsu_he_wire_build_query_request(uint8_t compression_type, const uint8_t *relin_keys, size_t relin_keys_size, uint32_t n_parts,
                                     const uint32_t *exponents, const uint32_t *cts_per_part, const uint8_t *const *ct_data,
                                     const size_t *ct_sizes, uint8_t **out, size_t *out_size);
/* ReceiverOperationQuery::load (receiver_operation.cpp:249-350): "unexpected operation type", "unsupported compression
 * mode", "invalid query data" (duplicate exponent) as in the reference */
int apsu_he_wire_parse_query_request(const uint8_t *buf, size_t size, apsu_he_wire_query **out);
int apsu_he_wire_query_free(apsu_he_wire_query *q);
int apsu_he_wire_query_info(const apsu_he_wire_query *q, uint8_t *compression_type, int *has_relin_keys, const uint8_t **relin_keys,
                            size_t *relin_keys_size, uint32_t *n_parts);
int apsu_he_wire_query_part(const apsu_he_wire_query *q, uint32_t part, uint32_t *exponent, uint32_t *n_cts);
int apsu_he_wire_query_ct(const apsu_he_wire_query *q, uint32_t part, uint32_t ct, const uint8_t **data, size_t *size);
int apsu_he_wire_build_query_response(uint32_t package_count, uint32_t alpha_max_cache_count, uint8_t **out, size_t *out_size);
int apsu_he_wire_parse_query_response(const uint8_t *buf, size_t size, uint32_t *package_count, uint32_t *alpha_max_cache_count);
/* ResultPackage::save / load (result_package.cpp:29-150) */
int apsu_he_wire_build_result_package(uint32_t bundle_idx, uint32_t cache_idx, const uint8_t *psu_result, size_t psu_result_size,
                                      uint32_t label_byte_count, uint32_t nonce_byte_count, uint32_t n_labels,
                                      const uint8_t *const *label_data, const size_t *label_sizes, uint8_t **out, size_t *out_size);
int apsu_he_wire_parse_result_package(const uint8_t *buf, size_t size, uint32_t *bundle_idx, uint32_t *cache_idx,
                                      const uint8_t **psu_result, size_t *psu_result_size, uint32_t *label_byte_count,
                                      uint32_t *nonce_byte_count, uint32_t *n_labels);
int apsu_he_wire_result_label(const uint8_t *buf, size_t size, uint32_t index, const uint8_t **data, size_t *data_size);
/* every label of a package with ONE parse (capacity 0: only *n_labels) */
int apsu_he_wire_result_labels(const uint8_t *buf, size_t size, uint32_t capacity, const uint8_t **data, size_t *sizes, uint32_t *n_labels);

/* ---- SEAL's own object serialisation: what is INSIDE Ciphertext.data / QueryRequest.relin_keys (host only, no GPU) ----
 * **UNPINNED**: restated from memory of upstream SEAL >= 3.6 / 4.x (apsu_amd/csrc/seal_codec.h lists every field); nothing in
 * the reference or this image can confirm it, the tests hold it against an independent Python model only (zlib and the BLAKE2b
 * core are pinned by python's zlib / hashlib).  Covers what the reference really puts on the wire
 * (sender/apsu/plaintext_powers.cpp:41-46, sender_osn.cpp:223-227,488, receiver/apsu/query.cpp:44-80, seal_object.h:161-219):
 *   - SEALHeader + body, compr_mode none, zlib or zstd (zstd through the system's libzstd.so.1, loaded at run time; refused with a
 *     clear message where that library is absent);
 *   - seeded ciphertexts (Serializable<Ciphertext> of encrypt_symmetric): c1 is expanded from the stored seed with SEAL's
 *     Blake2xb generator and util::sample_poly_uniform;
 *   - KSwitchKeys / RelinKeys (seeded or not) into the [decomp][2][K][n] array apsu_he_relin_upload takes;
 *   - parms_id = BLAKE2b-256 over {scheme, n, coeff moduli, plain modulus} for every level of the chain.
 * apsu_he_seal_ctx holds a parameter set's modulus chain; chain_idx as everywhere (K - 1 or -1 = the key level). */
typedef struct apsu_he_seal_ctx apsu_he_seal_ctx;
#define APSU_HE_SEAL_COMPR_NONE 0
#define APSU_HE_SEAL_COMPR_ZLIB 1
int apsu_he_seal_ctx_create(const char *psu_params_json, apsu_he_seal_ctx **out);
int apsu_he_seal_ctx_create_raw(uint64_t poly_modulus_degree, const uint64_t *coeff_modulus, int k, uint64_t plain_modulus,
                                apsu_he_seal_ctx **out);
int apsu_he_seal_ctx_free(apsu_he_seal_ctx *c);
int apsu_he_seal_parms_id(const apsu_he_seal_ctx *c, int chain_idx, uint64_t out[4]);
/* util::sample_poly_uniform under the Blake2xb generator seeded with seed[8]: out[L][n] at that level */
int apsu_he_seal_sample_poly_uniform(const apsu_he_seal_ctx *c, int chain_idx, const uint64_t seed[8], uint64_t *out);
/* Ciphertext::load: data receives size * L * n words ([poly][limb][coeff]), c1 expanded when the object was seeded.
 * c may be NULL for unseeded objects (chain_idx is then -1).  *consumed = bytes of the object. */
int apsu_he_seal_ct_load(const apsu_he_seal_ctx *c, const uint8_t *buf, size_t size, uint64_t parms_id[4], int *chain_idx, int *is_ntt_form,
                         uint64_t *ct_size, uint64_t *poly_modulus_degree, uint64_t *coeff_modulus_size, int *was_seeded, uint64_t *data,
                         size_t data_capacity_words, size_t *consumed);
/* The same WITHOUT expanding a seed: a seeded object yields c0 (L * n words), *was_seeded = 1 and seed[8] -- feed the seed to
 * apsu_he_seed_expand, which writes c1 into device memory; an unseeded object yields all its words. */
int apsu_he_seal_ct_load_unexpanded(const apsu_he_seal_ctx *c, const uint8_t *buf, size_t size, int *chain_idx, int *is_ntt_form,
                                    uint64_t *ct_size, uint64_t *coeff_modulus_size, int *was_seeded, uint64_t seed[8], uint64_t *data,
                                    size_t data_capacity_words, size_t *consumed);
/* Ciphertext::save at that level; seed != NULL writes the seeded form (c1 is NOT written: the caller guarantees it equals
 * apsu_he_seal_sample_poly_uniform(seed)) */
int apsu_he_seal_ct_save(const apsu_he_seal_ctx *c, int chain_idx, int is_ntt_form, uint64_t ct_size, const uint64_t *data, const uint64_t *seed,
                         int compr_mode, int version_major, int version_minor, uint8_t **out, size_t *out_size);
/* Plaintext::load / ::save (parms_id zero = coefficient form: *chain_idx = -1; else the level it was transformed at).  data NULL: only
 * the dimensions.  These are the objects a BinBundle's cache holds per coefficient (bin_bundle.cpp:421-428, compr none or zstd). */
int apsu_he_seal_pt_load(const apsu_he_seal_ctx *c, const uint8_t *buf, size_t size, int *chain_idx, uint64_t *coeff_count, uint64_t *data,
                         size_t data_capacity_words, size_t *consumed);
int apsu_he_seal_pt_save(const apsu_he_seal_ctx *c, int chain_idx, const uint64_t *data, uint64_t coeff_count, int compr_mode, int version_major,
                         int version_minor, uint8_t **out, size_t *out_size);
/* apsu_he_db_upload_bundle from the reference's own representation: blobs[d] / blob_sizes[d] = batched_coeffs[d].data() / .size() of
 * BatchedPlaintextPolyn (receiver/apsu/bin_bundle.h:52-134), i.e. SEAL-serialised Plaintexts; form and level are read from each
 * object's parms_id and checked against the rule of bin_bundle.cpp:385-389,418-420.  No SEAL on the host.  (ABI 4) */
int apsu_he_db_upload_bundle_serialized(apsu_he_ctx *ctx, const apsu_he_seal_ctx *seal_ctx, uint32_t bundle_idx, uint32_t cache_idx, uint32_t n_coeffs,
                                        const uint8_t *const *blobs, const size_t *blob_sizes, apsu_he_bundle **out);
/* The rest of the framing around the path (ABI 4).  apsu_he_wire_peek_type: the union tag of a ReceiverOperation (1 ParmsRequest,
 * 2 OPRFRequest, 3 QueryRequest, 4 plainResponse; rop.fbs) or of a ReceiverOperationResponse (1 ParmsResponse, 2 OPRFResponse,
 * 3 QueryResponse; rop_response.fbs).  The parameter exchange: ParmsRequest {} / ParmsResponse { data } with data = PSUParams::save's
 * bytes (psu_params.fbs + SEAL's EncryptionParameters object, psu_params.cpp:182-290): apsu_he_wire_psu_params_save turns the JSON
 * apsu_he_create takes into those bytes, _load turns them back into that JSON (explicit coefficient primes must be
 * CoeffModulus::Create's for their bit sizes, which is what every JSON-created parameter set has).  plainResponse { bundle_idx,
 * psu_result:[uint64], cache_idx }: the querier's decrypted results on their way back to the DB side (receiver_operation.cpp).
 * The EncryptionParameters object is restated from memory of upstream SEAL like the rest of apsu_he_seal_*: UNPINNED. */
int apsu_he_wire_peek_type(const uint8_t *buf, size_t size, int is_response, int *type);
int apsu_he_wire_psu_params_save(const char *psu_params_json, uint8_t **out, size_t *out_size);
int apsu_he_wire_psu_params_load(const uint8_t *buf, size_t size, uint8_t **psu_params_json, size_t *json_size);   /* not NUL-terminated */
int apsu_he_wire_build_parms_request(uint8_t **out, size_t *out_size);
int apsu_he_wire_build_parms_response(const uint8_t *psu_params, size_t psu_params_size, uint8_t **out, size_t *out_size);
int apsu_he_wire_parse_parms_response(const uint8_t *buf, size_t size, const uint8_t **psu_params, size_t *psu_params_size);   /* into buf */
int apsu_he_wire_build_plain_response(uint32_t bundle_idx, uint32_t cache_idx, const uint64_t *psu_result, size_t count, uint8_t **out, size_t *out_size);
int apsu_he_wire_parse_plain_response(const uint8_t *buf, size_t size, uint32_t *bundle_idx, uint32_t *cache_idx, uint64_t *psu_result, size_t capacity,
                                      size_t *count);
/* The header ReceiverDB::save writes in front of the BinBundles (receiver/apsu/receiver_db.fbs, receiver_db.cpp:1182-1232): the
 * parameters as JSON (release with apsu_he_wire_buffer_free; NULL: skip), item count, BinBundle count, flags; *consumed = offset of
 * the first BinBundle, to be walked with apsu_he_wire_bin_bundle_info / apsu_he_db_upload_saved_bundle below. */
int apsu_he_wire_receiver_db_header(const uint8_t *buf, size_t size, uint8_t **psu_params_json, size_t *json_size, uint64_t *item_count,
                                    uint32_t *bin_bundle_count, int *compressed, int *stripped, uint32_t *label_byte_count, size_t *consumed);
/* One BinBundle as the reference persists it: the size-prefixed FlatBuffers buffer BinBundle::save appends to a saved ReceiverDB
 * (receiver/apsu/bin_bundle.fbs; bin_bundle.cpp:1085-1168; ReceiverDB::save receiver_db.cpp:1182-1260 writes them one after the
 * other behind its own header).  apsu_he_wire_bin_bundle_info: its dimensions and *consumed = where the next one starts.
 * apsu_he_db_upload_saved_bundle: onto the device -- from the saved cache when there is one (SEAL Plaintext objects, read by the
 * codec above: seal_ctx required), else rebuilt from the item bins on the GPU (apsu_he_db_build_bundle); the checks of
 * BinBundle::load (bin_bundle.cpp:1170-1230: field modulus, number of bins, bin sizes) -> APSU_HE_RUNTIME_ERROR "failed to load
 * BinBundle".  Labels and interpolation polynomials are not read (the unlabeled protocol).  (ABI 4) */
int apsu_he_wire_bin_bundle_info(const uint8_t *buf, size_t size, uint32_t *bundle_idx, uint64_t *mod, int *stripped, uint32_t *n_bins,
                                 uint32_t *largest_bin, uint32_t *cache_coeffs, size_t *consumed);
int apsu_he_db_upload_saved_bundle(apsu_he_ctx *ctx, const apsu_he_seal_ctx *seal_ctx, const uint8_t *buf, size_t size, uint32_t cache_idx,
                                   apsu_he_bundle **out, size_t *consumed);
/* The way back: a resident database written in the reference's saved format, for the reference's receiver, a CPU fallback or its
 * tools.  (Additive to ABI 7.)
 *
 * The host writers.  apsu_he_wire_build_bin_bundle: one BinBundle as BinBundle::save writes it (bin_bundle.cpp:1107-1169).  A ragged
 * matrix arrives flat with n_rows + 1 offsets in words (row i = felts[offsets[i] .. offsets[i + 1])): the item bins, and the bins'
 * matching polynomials (ascending, monic; [1] for an empty bin).  Written: bundle_idx, mod, item_bins (no rows when stripped),
 * label_bins (present, empty), the cache unless has_cache is 0 { felt_matching_polyns (no rows when stripped), batched_matching_polyn
 * with coeffs[d] = the SEAL-serialised Plaintext of degree d, felt_interp_polyns and batched_interp_polyns (present, empty) },
 * stripped.  stripped without the cache is refused.  apsu_he_wire_build_receiver_db_header: the header ReceiverDB::save puts in front
 * (receiver_db.cpp:1182-1232); hashed_items is [n][2] = low, high word.  Both compute the exact size of their buffer first and refuse
 * one over 2^31 - 1 bytes (FlatBuffers offsets are 32 bit) before anything is allocated: APSU_HE_INVALID_ARGUMENT, the size named;
 * apsu_he_wire_saved_size_check is that bound alone.  The readers next to them: apsu_he_wire_receiver_db_header_fields (pointers into
 * buf), apsu_he_wire_bin_bundle_rows (which: 0 item_bins, 1 cache.felt_matching_polyns; felts / offsets NULL: only the counts),
 * apsu_he_wire_bin_bundle_coeffs (every plaintext of the cache with one parse, pointers into buf; data NULL: only *count) and apsu_he_wire_bin_bundle_extras (entries of the label-side vectors, -1 where absent). */
int apsu_he_wire_saved_size_check(uint64_t bytes);
int apsu_he_wire_build_bin_bundle(uint32_t bundle_idx, uint64_t mod, int stripped, int has_cache, const uint64_t *bin_felts, const uint64_t *bin_offsets,
                                  size_t n_bins, const uint64_t *polyn_felts, const uint64_t *polyn_offsets, size_t n_polyns, const uint8_t *const *coeffs,
                                  const size_t *coeff_sizes, uint32_t n_coeffs, uint8_t **out, size_t *out_size);
int apsu_he_wire_build_receiver_db_header(const uint8_t *psu_params, size_t psu_params_size, uint32_t label_byte_count, uint32_t nonce_byte_count,
                                          uint64_t item_count, int compressed, int stripped, const uint8_t *oprf_key, size_t oprf_key_size,
                                          const uint64_t *hashed_items, size_t n_hashed_items, uint32_t bin_bundle_count, uint8_t **out, size_t *out_size);
int apsu_he_wire_receiver_db_header_fields(const uint8_t *buf, size_t size, const uint8_t **psu_params, size_t *psu_params_size, const uint8_t **oprf_key,
                                           size_t *oprf_key_size, const uint8_t **hashed_items, size_t *n_hashed_items, uint32_t *nonce_byte_count);
int apsu_he_wire_bin_bundle_rows(const uint8_t *buf, size_t size, int which, uint64_t *felts, size_t felt_capacity, uint64_t *offsets, size_t offset_capacity,
                                 size_t *n_rows, size_t *n_felts);
int apsu_he_wire_bin_bundle_coeffs(const uint8_t *buf, size_t size, const uint8_t **data, size_t *data_sizes, uint32_t capacity, uint32_t *count);
int apsu_he_wire_bin_bundle_extras(const uint8_t *buf, size_t size, int *has_cache, int32_t *label_bins, int32_t *felt_interp_polyns,
                                   int32_t *batched_interp_polyns);
/* apsu_he_bundle_export_saved: a resident BinBundle -> that buffer (release with apsu_he_wire_buffer_free), such that
 * apsu_he_db_upload_saved_bundle of it has the apsu_he_bundle_save image of `bundle`, bit for bit, under every flag setting.  One
 * decode of the stored plaintexts serves everything: the item bins are apsu_he_bundle_bins', the matching polynomials are the
 * decoded columns cut to the bins' counts (k_bins_rows: a transposition on the device, so they leave it with one contiguous copy),
 * plaintext d is what the BatchedPlaintextPolyn ctor keeps (bin_bundle.cpp:366-430): coefficient form mod t with n coefficients and
 * a zero parms_id for d = 0 and, with Paterson-Stockmeyer, d % (ps_low_degree + 1) == 0 -- the decode's values before its forward
 * transform mod t -- else the stored rows [(pt_level + 1)][n] in NTT form under that level's parms_id; each is serialised by the
 * codec above (compr_mode 0 none or 2 zstd), one degree at a time.  flags: APSU_HE_SAVED_STRIPPED = what strip() leaves (no item
 * bins, no matching polynomials, stripped = true); APSU_HE_SAVED_NO_CACHE = the item bins alone; both together are refused.
 * Refused with APSU_HE_INVALID_ARGUMENT, the bin named in apsu_he_last_error, `bundle` untouched: unless stripped, a polynomial that
 * does not split into the bin's count of roots (apsu_he_bundle_bins' refusals: a BinBundle that was not built from bins), an unused
 * slot among the bins, a degree above every bin's count (BinBundle::load wants as many plaintexts as the longest matching polynomial
 * has coefficients; possible only for a BinBundle uploaded with plaintexts above its longest bin), and a bin of max_items_per_bin items (apsu_he_db_build_bundle allows it; BinBundle::load's cache check does
 * not); a buffer over the 32-bit limit.  What BinBundle::load checks and this writer meets: mod = the field modulus; unstripped,
 * exactly bins_per_bundle item bins of at most max_items_per_bin items and as many matching polynomials, the longest of at most
 * max_items_per_bin coefficients, and as many plaintexts as the longest has coefficients; stripped, a cache of at most
 * max_items_per_bin plaintexts; label sizes 0.  apsu_he_debug_export_times (next to apsu_he_debug_bins_times): the last call's times in ms -- decode and counts, root
 * search and multiplicities, k_bins_rows (device); copies to the host, serialisation, assembly (host).
 *
 * apsu_he_db_export_saved: the whole database into one file: the header (its compressed = compr_mode != 0, its stripped from flags),
 * then the BinBundles bundle-index-major, the caller's order kept within a bundle index, each exported, written and released before
 * the next.  Written to path + ".tmp" and renamed; a failing call leaves neither file.  The OPRF key and the hashed items are the
 * caller's (the engine never had them) and are written as given.  What ReceiverDB::Load checks (receiver_db.cpp:1257-1429) and the
 * call therefore requires: the buffer verifies; the parameters load (they are the context's own, apsu_he_wire_psu_params_save's
 * bytes); the OPRF key has 32 bytes, which Load copies whatever the vector's length (a stripped database may pass none: 32 zero
 * bytes are written); unstripped, item_count equals the number of hashed items; bin_bundle_count BinBundles follow, each passing
 * BinBundle::load with a bundle index below bundle_idx_count.  apsu_he_multi_db_export_saved: the same for the BinBundles of a
 * multi-device handle, in apsu_he_multi_db_index_bundles' order within a bundle index; every BinBundle is exported by the device
 * that owns it and the file is written by the calling thread. */
#define APSU_HE_SAVED_STRIPPED 1u
#define APSU_HE_SAVED_NO_CACHE 2u
int apsu_he_bundle_export_saved(apsu_he_ctx *ctx, const apsu_he_seal_ctx *seal_ctx, const apsu_he_bundle *bundle, uint32_t flags, int compr_mode,
                                uint8_t **out, size_t *out_size);
int apsu_he_debug_export_times(apsu_he_ctx *ctx, double *ms6);
int apsu_he_db_export_saved(apsu_he_ctx *ctx, const apsu_he_seal_ctx *seal_ctx, const char *path, const apsu_he_bundle *const *bundles, int count,
                            uint32_t flags, int compr_mode, const uint8_t *oprf_key, size_t oprf_key_size,
                            const uint64_t *hashed_items /* [n][2]: low, high */, size_t n_hashed_items, uint64_t item_count);
int apsu_he_multi_db_export_saved(apsu_he_multi *m, const apsu_he_seal_ctx *seal_ctx, const char *path, uint32_t flags, int compr_mode,
                                  const uint8_t *oprf_key, size_t oprf_key_size, const uint64_t *hashed_items, size_t n_hashed_items, uint64_t item_count);
/* RelinKeys::load -> ksk[K-1][2][K][n] (ksk NULL: only *words); ::save (seeds[K-1][8] or NULL) */
int apsu_he_seal_relin_keys_load(const apsu_he_seal_ctx *c, const uint8_t *buf, size_t size, uint64_t *ksk, size_t capacity_words, size_t *words,
                                 size_t *consumed);
int apsu_he_seal_relin_keys_save(const apsu_he_seal_ctx *c, const uint64_t *ksk, const uint64_t *seeds, int compr_mode, int version_major,
                                 int version_minor, uint8_t **out, size_t *out_size);
/* The seed expansion ON THE DEVICE (needs a GPU context): c1 of `count` seeded objects at chain_idx (-1 / K - 1 = key level)
 * = util::sample_poly_uniform under SEAL's Blake2xb generator seeded with seeds[i*8 .. i*8+7], written to the device buffers
 * dst_device[i] ([L][n] words).  Same values as apsu_he_seal_sample_poly_uniform (the host form costs ~0.2 ms per 384 KiB
 * ciphertext and core; 24 query ciphertexts expand in one launch pair here).  Synchronous. */
int apsu_he_seed_expand(apsu_he_ctx *ctx, int chain_idx, int count, const uint64_t *seeds, uint64_t *const *dst_device);
/* Receiver::RunQuery from the wire, without SEAL on the host (receiver_osn.cpp:160-364, query.cpp:44-80, result_package.cpp:29-76):
 * `request` = the size-prefixed ReceiverOperation{QueryRequest} buffer as ZMQChannel::receive_operation hands it over.  Its
 * RelinKeys are decoded and uploaded, every query ciphertext is decoded (c0 through page-locked memory, a seeded c1 expanded on
 * the device), ComputePowers runs for the bundle indices of the given BinBundles, every BinBundle is evaluated with its mask,
 * and packages[i] / package_sizes[i] receive one size-prefixed ResultPackage per BinBundle (result ciphertext as a SEAL object at
 * the last level under result_compr_mode; release each with apsu_he_wire_buffer_free).  Errors as the reference raises them:
 * exponents that do not match the parameters' query_powers, a wrong ciphertext count per exponent, missing RelinKeys -> 
 * APSU_HE_INVALID_ARGUMENT.  UNPINNED as far as SEAL's object format goes (apsu_he_seal_*). */
int apsu_he_run_query_request(apsu_he_ctx *ctx, const apsu_he_seal_ctx *seal_ctx, const uint8_t *request, size_t request_size,
                              const apsu_he_bundle *const *bundles, int count, const uint64_t *const *masks, int masks_on_device,
                              int result_compr_mode, uint8_t **packages, size_t *package_sizes);
/* The same for the multi-device handle: the request is decoded once onto the handle's first device (seeded c1
 * expanded there), its RelinKeys go to every device, the other devices fetch the ciphertexts of their bundle indices over xGMI, and
 * EVERY BinBundle registered in the handle gets its ResultPackage: packages[id] / package_sizes[id], capacity >= the handle's
 * BinBundle count.  masks[id]: host memory.  (ABI 4) */
int apsu_he_multi_run_query_request(apsu_he_multi *m, const apsu_he_seal_ctx *seal_ctx, const uint8_t *request, size_t request_size,
                                    const uint64_t *const *masks, int result_compr_mode, uint8_t **packages, size_t *package_sizes, int capacity);
/* round-2 entry points, kept: one unseeded ciphertext without a context (zlib bodies are inflated on load) */
int apsu_he_wire_seal_ct_save(const uint64_t parms_id[4], int is_ntt_form, uint64_t ct_size, uint64_t poly_modulus_degree,
                              uint64_t coeff_modulus_size, uint64_t correction_factor, double scale, const uint64_t *data,
                              int version_major, int version_minor, uint8_t **out, size_t *out_size);
int apsu_he_wire_seal_ct_load(const uint8_t *buf, size_t size, uint64_t parms_id[4], int *is_ntt_form, uint64_t *ct_size,
                              uint64_t *poly_modulus_degree, uint64_t *coeff_modulus_size, uint64_t *correction_factor, double *scale,
                              uint64_t *data, size_t data_capacity_words, int *version_major, int *version_minor);

/* ---- measurement hooks (replace the reference's STOPWATCH timers, receiver_osn.cpp:167,403,504) ----
 * Per-kernel-class device time from HIP events recorded on the engine's stream around each launch.
 * Classes (index): 0 ntt_fwd, 1 ntt_inv, 2 dyadic_mac, 3 behz_ext, 4 behz_tensor, 5 behz_finish,
 * 6 keyswitch, 7 modswitch, 8 other, 9 ntt_fused (inverse transforms whose load forms the BEHZ tensor product or the key
 * switch's inner product: k_intt_tensor, k_intt_ks).  units: limb polynomials for 0/1/9, plaintext limb-terms for 2.
 * mode 2 times classes 0, 1 and 9 only. */
#define APSU_HE_PROFILE_CLASSES 10
int apsu_he_profile_enable(apsu_he_ctx *ctx, int mode);   /* 0 off, 1 every class, 2 NTT launches only */
int apsu_he_profile_read(apsu_he_ctx *ctx, double *ms, uint64_t *launches, uint64_t *units, int capacity, int reset);

/* Phase timers under the reference's own STOPWATCH names (receiver_osn.cpp:167,403,504; report format cli/common_utils.cpp:54-76:
 * instances, average, minimum, maximum): 0 "Receiver::RunQuery" (start of apsu_he_compute_powers .. end of the last
 * apsu_he_eval_bundles before the next apsu_he_compute_powers), 1 "Receiver::ComputePowers", 2 "Receiver::ProcessBinBundleCache"
 * (one span per apsu_he_eval_bundles call, i.e. over ALL its BinBundles: they are evaluated as one batch).  Device time from
 * HIP events on the context's streams; enable costs two to five event records per call.  reset != 0 clears all three. */
#define APSU_HE_PHASES 3
const char *apsu_he_phase_name(int phase);
int apsu_he_phase_enable(apsu_he_ctx *ctx, int on);
int apsu_he_phase_read(apsu_he_ctx *ctx, int phase, uint64_t *count, double *avg_ms, double *min_ms, double *max_ms, int reset);

/* Host-side events inside the engine that cost a query time without being a kernel (diagnosis of launch-bound shards):
 * 0 host waits, 1 job-table uploads (cache misses), 2 job-table hits, 3 workspace-arena growths, 4 powers-buffer
 * allocations, 5 wraps of the pinned staging area, 6 job-table re-allocations, 7 (ABI 6) ComputePowers calls that were pipelined
 * with the evaluation in front (apsu_he_set_query_overlap).  Monotonic since apsu_he_create. */
#define APSU_HE_DEBUG_COUNTERS 8
int apsu_he_debug_counters(apsu_he_ctx *ctx, uint64_t *out, int capacity);

#ifdef __cplusplus
}
#endif
#endif /* APSU_HE_H */
