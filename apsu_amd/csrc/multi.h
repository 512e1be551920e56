// Several GPUs of one node behind one handle: the in-process counterpart of Receiver::RunQuery's fan-out of BinBundle
// tasks (receiver/apsu/receiver_osn.cpp:320-364).  One Engine per device, one persistent host thread per device;
// BinBundles are the sharded unit: devices are assigned to bundle indices first, an index's BinBundles
// are split over its devices by cost ~ degree (longest-processing-time greedy); every device computes the powers of
// its own indices only, and the only data exchange of a query is the final gather of the fixed-size results.
#pragma once
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "db_file.h"
#include "engine.h"
#include "multi_place.h"
#include "sharding.h"

namespace apsu_he {

class MultiEngine {
public:
    MultiEngine(const HeParams &hp, const PSUParams &psu, const std::vector<int> &devices);
    ~MultiEngine();
    MultiEngine(const MultiEngine &) = delete;
    MultiEngine &operator=(const MultiEngine &) = delete;

    int device_count() const { return (int)devs_.size(); }
    Engine &engine(int slot) { return *devs_.at(slot)->eng; }
    const PSUParams &psu() const { return psu_; }
    const HeParams &he() const { return hp_; }

    void upload_relin_keys(const u64 *ksk);                      // replicated on every device
    // the same with seeded keys: c1 of entry i (at word c1_at[i] of ksk) is sampled from seeds[i * 8 ..] on every device, in place
    void upload_relin_keys_seeded(const u64 *ksk, const u64 *seeds, const size_t *c1_at, int n_seeded);
    // DB placement: the bundle's id is its registration order (= its row in eval_all's output) until a maintenance call below renumbers
    int upload_bundle(int slot, uint32_t bundle_idx, uint32_t cache_idx, uint32_t n_coeffs, const u64 *const *coeff_ptrs,
                      const unsigned char *is_ntt);
    int random_bundle(int slot, uint32_t bundle_idx, uint32_t cache_idx, uint32_t degree, u64 seed);
    // N2: the whole DB from / to one file (db_file.h).  load_file places the file's BinBundles with the partition rule (spill pass
    // included) and every device reads its own shard from the shared mapping, all devices at once; ids = the file's table order,
    // appended to whatever is registered already.  Returns the number of BinBundles loaded.
    int load_file(const DbFile &f);
    void save_file(const std::string &path);                      // every registered BinBundle, in id order
    // the database in the reference's saved format (db_file.h: saved_db_export): every bundle index in turn, index_bundles' order within
    // it; each BinBundle is exported by the device that owns it, the file is written by the calling thread
    void export_saved_db(const std::string &path, const wire::ReceiverDbHeaderParts &header, const uint64_t ntt_parms_id[4], uint32_t flags, int compr);
    int bundle_count() const { return (int)where_.size(); }
    int bundle_device(int id) const { return where_.at(id).first; }
    const Bundle &bundle(int id) const { const auto &w = where_.at(id); return *devs_[w.first]->bundles[w.second]; }
    void clear_bundles();
    // Engine::update_bundle on BinBundle `id`, on its device; the new BinBundle takes its place (same id, same output row) once
    // that device has finished what was queued on the old one
    void update_bundle(int id, const u64 *ins_roots, const uint32_t *ins_counts, uint32_t ins_stride, const u64 *rem_roots,
                       const uint32_t *rem_counts, uint32_t rem_stride, uint32_t bins);

    // ---- the resident database maintained on the handle (multi_db.cpp).  The rules -- where a new BinBundle goes, every id after a
    // change, where a merge is made -- are multi_place.h's.  Every call takes the handle's lock, is synchronous and is all-or-nothing:
    // new BinBundles are built first, every owning engine is waited for (evaluations with device-side results may still read the old
    // rows), and only then are ids and rows committed; a call that throws leaves ids, count and results as they were.  Work of different
    // devices is queued on their workers at once.  After a call that drops BinBundles the ids are dense again: new_id[old id] is the
    // id a BinBundle has from now on, -1 for a dropped one.
    std::vector<RegUnit> registry();                              // per id: slot, bundle_idx, cache_idx, degree
    std::vector<int> index_bundles(uint32_t bundle_idx);          // the ids of one bundle index in cache order (index_in_cache_order)
    void bin_counts(int id, uint32_t *counts);                    // Engine::bin_counts on the owning device
    void bundle_bins(int id, u64 *roots, uint32_t *counts, uint32_t stride);   // Engine::bundle_bins on the owning device
    SelfTestReport self_test(const u64 seed[8]);                 // Engine::self_test of every device's BinBundles, the reports reduced (bin_eval.h)
    // Engine::build_bundle on `slot`, or with slot == -1 on the slot place_new_unit chooses; registered last.  Returns the id.
    int build_bundle(int slot, uint32_t bundle_idx, uint32_t cache_idx, const u64 *roots, const uint32_t *counts, uint32_t bins, uint32_t stride);
    void remove_bundle(int id, int *new_id);                      // new_id[bundle_count()] (may be null)
    // the BinBundle's arrays go device to device (Engine::clone_bundle); the id stays.  A move to its own slot does nothing.
    void move_bundle(int id, int slot);
    // Engine::lookup_bundles against index_bundles(bundle_idx), rows in that order; every device looks up its own BinBundles
    void lookup(uint32_t bundle_idx, const u64 *felts, const uint32_t *start, size_t count, unsigned char *present, uint32_t *room);
    struct ApplyOutcome {
        PlaceResult place;                                        // targets: positions among index_bundles(bundle_idx), then the appended ones
        std::vector<int> ids;                                     // index_bundles(bundle_idx) before the call
        int old_count = 0;                                        // bundle_count() before the call: the k-th appended BinBundle is old id old_count + k
        std::vector<int> new_id;                                  // [old_count + place.n_new]
    };
    // Engine::apply_entries' contract on index_bundles(bundle_idx): per-device lookup, place_entries on the host, update_bundle per
    // changed BinBundle on its device, build_bundle per appended one on the slot place_new_unit gives it (loads taken after the updates,
    // the EMPTY BinBundles still counted; appended ones placed in order), EMPTY BinBundles dropped, ids renumbered
    ApplyOutcome apply_entries(uint32_t bundle_idx, const u64 *ins_felts, const uint32_t *ins_start, size_t n_ins, const u64 *rem_felts,
                               const uint32_t *rem_start, size_t n_rem);
    // Engine::build_from_entries on the handle (host entries): the plan once on the host, BinBundle (b, k) on the slot place_new_unit gives
    // it, in (b, k) order, the loads taken as each one registers; every device copies the entries of the bundle indices it builds for.
    // Refuses a handle that holds a BinBundle of a bundle index that receives entries.  -> (first id, BinBundles built), ids dense
    std::pair<int, uint32_t> build_from_entries(const unsigned char *entries, const u64 *offsets);
    // Engine::merge_bundles on the given BinBundles of one bundle index, wherever they lie: members that are not on merge_home travel
    // there as temporaries; the merged BinBundle takes the first member's (cache order) id slot and cache_idx, the others are dropped
    void merge_bundles(const int *ids, uint32_t n_ids, int *new_id);
    // counts per BinBundle on its device, plan_compaction on the host, one merge per group of two or more.  Returns the BinBundles made.
    uint32_t compact(uint32_t bundle_idx, int *new_id);

    // One query.  src_cts[b * source_count + s]: ciphertexts of every bundle index (each device reads its own);
    // masks[id]: n words mod t; out: bundle_count * 2n words, row = bundle id — host memory when out_slot < 0, else device
    // memory on devices[out_slot] (gathered over xGMI: peer copies, or one RCCL all-gather with IO_GATHER_RCCL).
    // flags: where the caller's buffers live.  Host buffers are pageable unless flagged page-locked (IO_*_PINNED: DMA goes
    // straight from / to them; pageable ones are staged through the device's own page-locked area, copy and DMA pipelined).
    // IO_SRC_ON_DEVICE / IO_MASKS_ON_DEVICE: the pointers are device pointers on devices[in_slot] (other devices fetch
    // what they need with peer copies).  Everything of a device's share is queued on its streams before the first wait.
    enum : unsigned { IO_SRC_PINNED = 1, IO_MASKS_PINNED = 2, IO_OUT_PINNED = 4, IO_SRC_ON_DEVICE = 8, IO_MASKS_ON_DEVICE = 16,
                      IO_GATHER_RCCL = 32 };
    void eval_all(const u64 *const *src_cts, const u64 *const *masks, u64 *out, int out_slot, unsigned flags = 0, int in_slot = 0);
    // what the last device-side gather used: "peer" or "rccl" ("" before the first one / host destination)
    const char *last_gather() const { return last_gather_; }
    // phase timers (Engine::phase_*): RunQuery = host wall time of eval_all; the other two = the slowest device's
    void phase_enable(bool on);
    void phase_read(Engine::PhaseSummary *out, bool reset);

private:
    struct Dev {
        int device = 0, slot = 0;
        std::unique_ptr<Engine> eng;
        std::unique_ptr<RelinKeys> rk;
        std::vector<std::unique_ptr<Bundle>> bundles;
        std::vector<int> ids;                                     // global id of bundles[i]
        DevBuf out;                                               // [bundles][2n] results of this device
        void *host_out = nullptr;                                 // pinned staging of the same size
        size_t host_out_bytes = 0;
        DevBuf in;                                                // this device's query inputs: sources, then masks
        void *host_in = nullptr;                                  // pinned staging for pageable inputs
        size_t host_in_bytes = 0;
        DevBuf gath;                                              // RCCL all-gather destination [devices][max rows][2n]
        // worker
        std::thread th;
        std::mutex mu;
        std::condition_variable cv;
        std::function<void()> job;
        bool has_job = false, done = false, quit = false;
        std::exception_ptr error;
    };
    void run_all(const std::function<void(Dev &)> &fn);
    // (multi_db.cpp; all of them with mu_ held)
    std::vector<RegUnit> registry_locked() const;
    const Bundle &bundle_locked(int id) const { const auto &w = where_.at((size_t)id); return *devs_[w.first]->bundles[w.second]; }
    void check_id(int id) const;
    struct Change;                                                // what a call replaces, drops and appends
    void commit(Change &c, int *new_id, std::vector<int> *new_id_out);
    std::vector<std::unique_ptr<Bundle>> merge_groups(const std::vector<std::vector<int>> &groups);
    static void worker(Dev *d);

    HeParams hp_;
    PSUParams psu_;
    std::vector<std::unique_ptr<Dev>> devs_;
    std::vector<std::pair<int, int>> where_;                      // id -> (slot, local position)
    std::mutex mu_;                                               // one query / placement call at a time
    const char *last_gather_ = "";
    // RCCL (librccl.so, loaded on first use): one communicator per device slot of this handle, null when unavailable
    struct Rccl;
    std::unique_ptr<Rccl> rccl_;
    bool rccl_tried_ = false;
    bool rccl_ready();
    bool phase_on_ = false;
    Engine::PhaseSummary run_query_;
};

} // namespace apsu_he
