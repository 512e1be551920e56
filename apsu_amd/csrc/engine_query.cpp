// The Engine's calls around a query: seeded objects expanded on the device (N3), masks, block packing and the loopback decryption
// (N4), and the querier's side -- key generation and query encryption (N5; query_side.h).
#include "engine_impl.h"
#include "seal_codec.h"

#include <functional>

namespace apsu_he {

// ============================================================================ N3: seeded objects expanded on the device
void Engine::seed_expand(int chain_idx, int count, const u64 *seeds, u64 *const *dst)
{
    Enter g(this);
    if (count <= 0) return;
    if (!seeds || !dst) throw std::invalid_argument("null argument");
    const bool key_level = chain_idx < 0 || chain_idx == hp_.K - 1;
    if (!key_level) check_level(chain_idx);
    for (int i = 0; i < count; i++) if (!dst[i]) throw std::invalid_argument("null destination");
    const int L = key_level ? hp_.K : chain_idx + 1;
    TIER1_SLOTS();
    job_seq_ = job_seq_base_;
    // The device list holds SEED_REJ_CAP = 8192 rejected words per object (APSU_HE_SEED_REJ_CAP lowers it: tests).  A word is refused
    // with probability (2^64 mod q) / 2^64: below 2^-27 for the primes 2^b - c a parameter file gives, up to ~q / 2^64 for a caller's own
    // primes (apsu_he_create_raw), so a large L * n of those may exceed the list (and L may exceed the device tables): such objects are
    // expanded by the host's sample_poly_uniform (seal_codec.cpp) and uploaded -- slower, same words.
    // APSU_HE_SEED_EXPAND_HOST=1 forces that path (tests).
    bool on_device = queue_seed_expand(L, count, seeds, dst);
    if (on_device) {
        sync();
        on_device = !seeds_overflowed(count);                    // more rejected words than the device list holds: the host redoes these objects
    }
    if (!on_device) host_seed_expand(L, count, seeds, dst);
}

// ============================================================================ N4: masks, packing, loopback decrypt
static uint32_t plain_modulus_len(u64 t)
{
    // receiver_osn.cpp:54-57: smallest len with (1 << len) - 1 >= plain_modulus
    uint32_t len = 1;
    while ((((u64)1 << len) - 1) < t) len++;
    return len;
}

void Engine::mask_generate(u64 seed, uint32_t count, u64 *masks_dev, u64 *values_host, u64 *blocks_host)
{
    mask_generate_impl(count, masks_dev, values_host, blocks_host, [&](u64 *vals, size_t words) { launch_fill_random(vals, words, seed, hp_.t, st_); });
}

void Engine::mask_generate_blake2xb(const u64 seed[8], u64 first_value, uint32_t count, u64 *masks_dev, u64 *values_host, u64 *blocks_host)
{
    Blake2xbSeed sd;
    for (int i = 0; i < 8; i++) sd.w[i] = seed[i];
    mask_generate_impl(count, masks_dev, values_host, blocks_host,
                       [&](u64 *vals, size_t words) { launch_fill_blake2xb(vals, words, sd, first_value, hp_.t, st_); });
}

void Engine::mask_generate_impl(uint32_t count, u64 *masks_dev, u64 *values_host, u64 *blocks_host, const std::function<void(u64 *, size_t)> &fill)
{
    Enter g(this);
    if (!has_psu_) throw std::logic_error("context was created without PSUParams");
    if (!hp_.batching) throw std::logic_error("plain_modulus does not support batching");
    if (!count) return;
    const size_t n = hp_.n;
    const uint32_t items = psu_.items_per_bundle, felts = psu_.item_params.felts_per_item;
    const int tid = hp_.plain_id();
    TIER1_SLOTS();
    WITH_ARENA({
        u64 *vals = ws((size_t)count * n);
        { PROF(P_OTHER, 0); fill(vals, (size_t)count * n); }                                                       // :248-251
        // BatchEncoder::encode (:271): slot permutation, inverse negacyclic NTT mod t
        { PROF(P_OTHER, 0); launch_scatter_slots(vals, reinterpret_cast<const uint32_t *>(d_slot_map_.p()), masks_dev, n, (int)count, st_); }
        d_ntt(masks_dev, count, map_ct() + tid, 1, true, false);
        if (blocks_host) {                                                                                        // :256-266
            u64 *blk = ws((size_t)count * items * 2);
            { PROF(P_OTHER, 0); launch_pack_blocks(vals, n, items, felts, plain_modulus_len(hp_.t), blk, (int)count, st_); }
            D2H(blocks_host, blk, (size_t)count * items * 2);
        }
        if (values_host) D2H(values_host, vals, (size_t)count * n);
        sync();
    });
}

void Engine::decrypt_decode(const u64 *sk_ntt_host, const u64 *cts, bool on_device, uint32_t count, u64 *values_host, u64 *blocks_host, int *budget_bits,
                            bool sk_on_device, u64 *values_dev)
{
    Enter g(this);
    if (!has_psu_) throw std::logic_error("context was created without PSUParams");
    if (!hp_.batching) throw std::logic_error("plain_modulus does not support batching");
    if (!count) return;
    const size_t n = hp_.n;
    const uint32_t items = psu_.items_per_bundle, felts = psu_.item_params.felts_per_item;
    const int tid = hp_.plain_id();
    for (size_t k = 0; !sk_on_device && k < n; k++)
        if (sk_ntt_host[k] >= hp_.key_q[0]) throw std::invalid_argument("secret key is not reduced modulo q_0");
    TIER1_SLOTS();
    WITH_ARENA({
        const u64 *sk = sk_ntt_host;                             // (sk_on_device: the engine's own key, used where it lies)
        if (!sk_on_device) {
            u64 *staged = ws(n);
            H2D(staged, sk_ntt_host, n);
            sk = staged;
        }
        const u64 *ct = cts;
        if (!on_device) {
            u64 *c = ws((size_t)count * 2 * n);
            H2D(c, cts, (size_t)count * 2 * n);
            ct = c;
        }
        // c1 -> NTT, (.) s, INTT  (dot_product_ct_sk_array at one limb)
        u64 *v = ws((size_t)count * n);
        std::vector<CtJob> cj;
        for (uint32_t i = 0; i < count; i++) cj.push_back(CtJob{ ct + ((size_t)i * 2 + 1) * n, v + (size_t)i * n });
        { PROF(P_OTHER, 0); launch_copy_jobs(upload_jobs(cj), n, (int)count, st_); }
        d_ntt(v, count, map_ct(), 1, false, data_primes_narrow_);
        { PROF(P_OTHER, 0); launch_dyadic_plain(dlevel(0), v, sk, v, 1, n, (int)count, 0, st_); }
        d_ntt(v, count, map_ct(), 1, true, data_primes_narrow_);
        // x = c0 + v; m = round(t x / q_0) mod t
        u64 *pt = ws((size_t)count * n);
        std::vector<u64> worst_host;
        if (budget_bits) {
            u64 *worst = ws(count);
            worst_host.resize(count);
            HIP_CHECK(hipMemsetAsync(worst, 0, count * sizeof(u64), st_));
            { PROF(P_OTHER, 0); launch_decrypt_round_budget(ct, 2 * n, v, hp_.key_q[0], hp_.t, pt, n, (int)count, worst, st_); }
            D2H(worst_host.data(), worst, count);
        } else
        { PROF(P_OTHER, 0); launch_decrypt_round(ct, 2 * n, v, hp_.key_q[0], hp_.t, pt, n, (int)count, st_); }
        // BatchEncoder::decode: forward NTT mod t, slot gather
        d_ntt(pt, count, map_ct() + tid, 1, false, false);
        u64 *vals = ws((size_t)count * n);
        { PROF(P_OTHER, 0); launch_gather_slots(pt, reinterpret_cast<const uint32_t *>(d_slot_map_.p()), vals, n, (int)count, st_); }
        if (blocks_host) {                                                                      // sender_osn.cpp:684-690
            u64 *blk = ws((size_t)count * items * 2);
            { PROF(P_OTHER, 0); launch_pack_blocks(vals, n, items, felts, plain_modulus_len(hp_.t), blk, (int)count, st_); }
            D2H(blocks_host, blk, (size_t)count * items * 2);
        }
        if (values_host) D2H(values_host, vals, (size_t)count * n);
        if (values_dev) D2D(values_dev, vals, (size_t)count * n);
        sync();
        // Decryptor::invariant_noise_budget: the largest b with worst 2^b < q_0, worst = max |t x mod q_0| centred, i.e.
        // ceil(log2(q_0 / (2 worst))); the bit count of q_0 for a noiseless result (worst = 0)
        for (uint32_t i = 0; budget_bits && i < count; i++) {
            const unsigned __int128 q0 = hp_.key_q[0], w = worst_host[i];
            int bits = 0;
            while (w && (w << (bits + 1)) < q0) bits++;
            budget_bits[i] = w ? bits : 64 - __builtin_clzll(hp_.key_q[0]);
        }
    });
}

// ============================================================================ N5: the querier's side (query_side.h)
void Engine::check_key_residues(const u64 *sk, int limbs) const
{
    for (int j = 0; j < limbs; j++)
        for (size_t k = 0; k < hp_.n; k++)
            if (sk[(size_t)j * hp_.n + k] >= hp_.key_q[j]) throw std::invalid_argument("secret key is not reduced modulo its limb's prime");
}

static Blake2xbSeed master_seed(const u64 seed[8])
{
    Blake2xbSeed sd;
    for (int i = 0; i < 8; i++) sd.w[i] = seed[i];
    return sd;
}

void Engine::host_seed_expand(int L, int count, const u64 *seeds, u64 *const *dst)
{
    std::vector<u64> q(hp_.key_q.begin(), hp_.key_q.begin() + L), buf((size_t)L * hp_.n);
    for (int i = 0; i < count; i++) {
        sealio::sample_poly_uniform(seeds + (size_t)i * 8, q.data(), (size_t)L, hp_.n, buf.data());
        HIP_CHECK(hipMemcpyAsync(dst[i], buf.data(), buf.size() * sizeof(u64), hipMemcpyHostToDevice, st_));
        sync();                                                  // buf is reused
    }
}

const DevLevel *Engine::seed_level(int L)
{
    const bool key_view = L == hp_.K && !key_level_.empty();     // the key level is not a data level: its moduli-only view (engine.h)
    if (key_view && !d_key_level_.p()) {
        d_key_level_.alloc(sizeof(DevLevel));
        HIP_CHECK(hipMemcpy(d_key_level_.p(), key_level_.data(), sizeof(DevLevel), hipMemcpyHostToDevice));
    }
    return key_view ? reinterpret_cast<const DevLevel *>(d_key_level_.p()) : dlevel(L - 1);
}

bool Engine::queue_seed_expand(int L, int count, const u64 *seeds, u64 *const *dst)
{
    if (L > DMAXL || sw_.seed_expand_host) return false;
    const DevLevel *lv = seed_level(L);
    const std::vector<u64> mm(max_multiple_.begin(), max_multiple_.begin() + L);
    std::vector<SeedJob> jobs(count);
    for (int i = 0; i < count; i++) {
        for (int k = 0; k < 8; k++) jobs[i].seed.w[k] = seeds[(size_t)i * 8 + k];
        jobs[i].dst = dst[i];
    }
    const size_t need = ((size_t)count * (1 + SEED_REJ_CAP) + 1) * sizeof(u32);
    if (d_seed_rej_.bytes() < need) {
        sync();
        d_seed_rej_.alloc(need * 2);
        HIP_CHECK(hipMemsetAsync(d_seed_rej_.p(), 0, d_seed_rej_.bytes(), st_));
    }
    u32 *rej = reinterpret_cast<u32 *>(d_seed_rej_.p());
    int *overflow = reinterpret_cast<int *>(rej + (size_t)count * (1 + SEED_REJ_CAP));
    HIP_CHECK(hipMemsetAsync(overflow, 0, sizeof(int), st_));
    { PROF(P_OTHER, 0); launch_seed_expand(upload_jobs(jobs), count, lv, L, upload_jobs(mm), hp_.n, rej, (u32)sw_.seed_rej_cap, overflow, st_); }
    return true;
}

// after a sync: did some object reject more words than the device lists hold?  (then the lists are cleared for their next use)
bool Engine::seeds_overflowed(int count)
{
    int h = 0;
    HIP_CHECK(hipMemcpy(&h, reinterpret_cast<u32 *>(d_seed_rej_.p()) + (size_t)count * (1 + SEED_REJ_CAP), sizeof(int), hipMemcpyDeviceToHost));
    if (h) {
        HIP_CHECK(hipMemsetAsync(d_seed_rej_.p(), 0, d_seed_rej_.bytes(), st_));
        sync();
    }
    return h != 0;
}

void Engine::keygen(const u64 seed[8], u64 *sk_ntt_host, bool sk_on_device)
{
    Enter g(this);
    const size_t n = hp_.n;
    const int K = hp_.K;
    TIER1_SLOTS();
    WITH_ARENA({
        signed char *small = reinterpret_cast<signed char *>(ws(n / 8));
        u64 *sk = ws((size_t)K * n);
        { PROF(P_OTHER, 0); launch_sample_ternary(master_seed(seed), small, n, st_); }
        { PROF(P_OTHER, 0); launch_small_lift(dkey(), small, sk, K, n, 1, st_); }
        d_ntt(sk, K, map_ct(), K, false, data_primes_narrow_);
        HIP_CHECK(hipMemcpyAsync(sk_ntt_host, sk, (size_t)K * n * sizeof(u64), sk_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st_));
        sync();
    });
}

void Engine::relin_keygen(const u64 *sk_ntt_host, const u64 seed[8], u64 *ksk_host, u64 *seeds_host, std::unique_ptr<RelinKeys> *resident, bool sk_on_device)
{
    Enter g(this);
    if (!hp_.using_keyswitching) throw std::invalid_argument("parameters do not support key switching: the reference creates no relinearisation keys");
    const size_t n = hp_.n;
    const int K = hp_.K, nk = K - 1;
    if (!sk_on_device) check_key_residues(sk_ntt_host, K);
    const Blake2xbSeed master = master_seed(seed);
    std::vector<u64> seeds((size_t)nk * 8);
    for (int i = 0; i < nk; i++) blake2xb_stream_block(master, qs_seed_block((u64)i), seeds.data() + (size_t)i * 8);
    auto rk = std::make_unique<RelinKeys>();
    const size_t words = (size_t)nk * 2 * K * n;
    rk->data.alloc(words * sizeof(u64));
    std::vector<u64 *> a(nk);
    for (int i = 0; i < nk; i++) a[i] = rk->data.u() + ((size_t)i * 2 + 1) * K * n;
    TIER1_SLOTS();
    WITH_ARENA({
        const u64 *sk = sk_ntt_host;
        if (!sk_on_device) {
            u64 *staged = ws((size_t)K * n);
            HIP_CHECK(hipMemcpyAsync(staged, sk_ntt_host, (size_t)K * n * sizeof(u64), hipMemcpyHostToDevice, st_));
            sk = staged;
        }
        signed char *small = reinterpret_cast<signed char *>(ws((size_t)nk * n / 8));
        u64 *e = ws((size_t)nk * K * n);
        bool on_device = queue_seed_expand(K, nk, seeds.data(), a.data());
        if (!on_device) host_seed_expand(K, nk, seeds.data(), a.data());
        auto rest = [&] {
            { PROF(P_OTHER, 0); launch_sample_cbd(master, 0, small, n, nk, st_); }
            { PROF(P_OTHER, 0); launch_small_lift(dkey(), small, e, K, n, nk, st_); }
            d_ntt(e, (size_t)nk * K, map_ct(), K, false, data_primes_narrow_);
            { PROF(P_OTHER, 0); launch_rlk_finish(dkey(), K, sk, e, rk->data.u(), n, st_); }
            sync();
        };
        rest();
        if (on_device && seeds_overflowed(nk)) {                 // (seed_expand's fallback: the host redoes the public halves)
            host_seed_expand(K, nk, seeds.data(), a.data());
            rest();
        }
    });
    if (ksk_host) HIP_CHECK(hipMemcpy(ksk_host, rk->data.p(), words * sizeof(u64), hipMemcpyDeviceToHost));
    if (seeds_host) std::memcpy(seeds_host, seeds.data(), seeds.size() * sizeof(u64));
    if (resident) *resident = std::move(rk);
}

void Engine::query_create(const u64 *sk_ntt_host, const u64 seed[8], const uint32_t *bundle_indices, int nb, const u64 *values, bool values_on_device,
                          u64 *cts_dev, u64 *seeds_host, bool sk_on_device)
{
    Enter g(this);
    if (!has_psu_) throw std::logic_error("context was created without PSUParams");
    if (!hp_.batching) throw std::logic_error("plain_modulus does not support batching");
    if (nb <= 0) return;
    const size_t n = hp_.n;
    const int first = hp_.first_chain_idx, L = first + 1, tid = hp_.plain_id();
    std::vector<u32> exps(psu_.query_params.query_powers.begin(), psu_.query_params.query_powers.end());   // ascending (std::set)
    const int S = (int)exps.size(), count = nb * S;
    if ((size_t)nb * S > 65535) throw std::invalid_argument("more than 65535 ciphertexts in one call");
    for (int b = 0; b < nb; b++)
        if (bundle_indices[b] >= psu_.bundle_idx_count) throw std::invalid_argument("bundle index out of range");
    if (!sk_on_device) check_key_residues(sk_ntt_host, L);
    if (!values_on_device)
        for (size_t i = 0; i < (size_t)nb * n; i++)
            if (values[i] >= hp_.t) throw std::invalid_argument("slot value is not reduced modulo the plain modulus");
    const Blake2xbSeed master = master_seed(seed);
    std::vector<u64> seeds((size_t)count * 8);
    for (int c = 0; c < count; c++) blake2xb_stream_block(master, qs_seed_block(QS_KEY_OBJECTS + (u64)c), seeds.data() + (size_t)c * 8);
    std::vector<u64 *> c1(count);
    for (int c = 0; c < count; c++) c1[c] = cts_dev + ((size_t)c * 2 + 1) * L * n;
    u32 flags_host = 0;
    TIER1_SLOTS();
    WITH_ARENA({
        const u64 *sk = sk_ntt_host;
        if (!sk_on_device) {
            u64 *staged = ws((size_t)L * n);
            HIP_CHECK(hipMemcpyAsync(staged, sk_ntt_host, (size_t)L * n * sizeof(u64), hipMemcpyHostToDevice, st_));
            sk = staged;
        }
        const u64 *vals = values;
        if (!values_on_device) {
            u64 *staged = ws((size_t)nb * n);
            HIP_CHECK(hipMemcpyAsync(staged, values, (size_t)nb * n * sizeof(u64), hipMemcpyHostToDevice, st_));
            vals = staged;
        }
        u32 *flags = reinterpret_cast<u32 *>(ws(1));
        HIP_CHECK(hipMemsetAsync(flags, 0, sizeof(u64), st_));
        u64 *pt = ws((size_t)count * n);
        signed char *small = reinterpret_cast<signed char *>(ws((size_t)count * n / 8));
        u64 *v = ws((size_t)count * L * n);
        // PlaintextPowers + BatchEncoder::encode (plaintext_powers.cpp:41-46,51-99)
        { PROF(P_OTHER, 0); launch_plain_powers(vals, reinterpret_cast<const uint32_t *>(d_slot_map_.p()), upload_jobs(exps), S, make_mod(hp_.t), pt, n, nb, flags, st_); }
        d_ntt(pt, count, map_ct() + tid, 1, true, false);
        { PROF(P_OTHER, 0); launch_sample_cbd(master, QS_KEY_OBJECTS, small, n, count, st_); }
        // Encryptor::encrypt_symmetric: c1 from its public seed, v = c1 s, c0 = Delta(m) - e - v
        bool on_device = queue_seed_expand(L, count, seeds.data(), c1.data());
        if (!on_device) host_seed_expand(L, count, seeds.data(), c1.data());
        auto rest = [&] {
            std::vector<const u64 *> src((size_t)count * L);
            for (int c = 0; c < count; c++)
                for (int j = 0; j < L; j++) src[(size_t)c * L + j] = c1[c] + (size_t)j * n;
            bool nored = hp_.logn <= 14;                         // (limb j of c1 is a canonical residue of q_j: nothing to reduce)
            for (int j = 0; j < L && nored; j++) nored = ntt_gather_nored_ok(hp_.key_q[j], hp_.key_q[j], hp_.logn);
            { PROF(P_NTT_FWD, src.size());
              launch_ntt_gather(hp_.logn, upload_jobs(src), v, src.size(), tabs(), map_ct(), L, st_, nored, sw_.ntt_latency_limbs, data_primes_narrow_); }
            { PROF(P_OTHER, 0); launch_dyadic_plain(dlevel(first), v, sk, v, 1, n, count, 0, st_); }
            d_ntt(v, (size_t)count * L, map_ct(), L, true, data_primes_narrow_);
            { PROF(P_OTHER, 0); launch_enc_finish(dlevel(first), pt, v, small, cts_dev, n, count, st_); }
            HIP_CHECK(hipMemcpyAsync(&flags_host, flags, sizeof(u32), hipMemcpyDeviceToHost, st_));
            sync();
        };
        rest();
        if (on_device && seeds_overflowed(count)) {
            host_seed_expand(L, count, seeds.data(), c1.data());
            rest();
        }
    });
    if (flags_host & QS_FLAG_VALUE) throw std::invalid_argument("slot value is not reduced modulo the plain modulus");
    if (seeds_host) std::memcpy(seeds_host, seeds.data(), seeds.size() * sizeof(u64));
}

} // namespace apsu_he
