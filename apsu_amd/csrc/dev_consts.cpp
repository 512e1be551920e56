// See dev_consts.h.  Host arithmetic only; part of the engine library and of the CPU emulation library.
#include "dev_consts.h"
#include "eval_plan.h"
#include "mac_core.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>

namespace apsu_he {

uint32_t packed_row_bits(u64 q)
{
    const int bits = 64 - __builtin_clzll(q);
    for (u32 c = (u32)std::max(bits, 32); c < 64; c++) {
        u32 g = 2 * c, r = 32;
        while (r) { const u32 t2 = g % r; g = r; r = t2; }
        if ((32 - g) + 2 * c <= 128) return c;
    }
    return 64;
}

// table reference of element `off` (dev_consts.h: DeviceConstants), and its resolution against the table's address
template <class T> static const T *table_ref(size_t off) { return reinterpret_cast<const T *>((uintptr_t)(off + 1)); }
template <class T, class B> static void resolve(const T *&p, const B *base)
{
    static_assert(sizeof(T) == 16 && sizeof(B) == 16, "table elements are 16 bytes");
    if (p) p = reinterpret_cast<const T *>(base) + (reinterpret_cast<uintptr_t>(p) - 1);
}

void DeviceConstants::relocate(const TwPair *tw_base, const ShoupConst *fin_base, const ShoupConst *drop_base, const ShoupConst *mdtw_base)
{
    for (NttTable &tb : tabs) { resolve(tb.fwd, tw_base); resolve(tb.dit, tw_base); resolve(tb.scale, tw_base); }
    for (DevLevel &d : levels) {
        for (int j = 0; j < DMAXL; j++) { resolve(d.fin_q[j], fin_base); resolve(d.drop_tw[j], drop_base); }
        for (int i = 0; i < DMAXB; i++) resolve(d.fin_b[i], fin_base);
        resolve(d.last_tw, tw_base);
    }
    for (int j = 0; j < DMAXL; j++) resolve(key.md_tw[j], mdtw_base);
    resolve(key.p_tw, tw_base);
}

// twiddles: per modulus [fwd n][dit n][scale n] TwPair, and the tables that name them
static void build_transform_tables(const HeParams &hp, DeviceConstants &dc)
{
    // the NTT keeps one limb in a workgroup's LDS: n = 2^logn coefficients with a compiled pass plan (ntt_core.h)
    // (32768: the limb is split into two LDS-resident halves around one radix-2 stage over global memory, kernels_ntt.hip)
    const bool split_ntt = hp.logn == 15;
    if (plan_passes(hp.logn) == 0 && !split_ntt)
        throw std::invalid_argument("poly_modulus_degree " + std::to_string(hp.n) +
                                    " is not supported by the GPU engine (supported: 64, 256, 1024, 2048, 4096, 8192, 16384, 32768)");
    const size_t n = hp.n;
    const int nmod = (int)hp.ntt.size();
    std::vector<TwPair> &tw = dc.tw;
    tw.resize((size_t)nmod * 3 * n + (split_ntt ? (size_t)nmod * n : 0));
    dc.tabs.resize(split_ntt ? (size_t)nmod * 2 : (size_t)nmod);
    const size_t halves = (size_t)nmod * 3 * n;                  // first element of the split transform's forward tables
    for (int m = 0; m < nmod; m++) {
        const NttTablesHost &t = hp.ntt[m];
        for (size_t k = 0; k < n; k++) {
            tw[((size_t)m * 3 + 0) * n + k] = TwPair{ t.fwd[k], t.fwd_q[k] };
            tw[((size_t)m * 3 + 1) * n + k] = TwPair{ t.dit[k], t.dit_q[k] };
            tw[((size_t)m * 3 + 2) * n + k] = TwPair{ t.scale[k], t.scale_q[k] };
        }
        NttTable tb = make_ntt_table(t, split_ntt ? hp.logn - 1 : hp.logn,           // stages inside one workgroup
                                     table_ref<TwPair>(((size_t)m * 3 + 0) * n), table_ref<TwPair>(((size_t)m * 3 + 1) * n),
                                     table_ref<TwPair>(((size_t)m * 3 + 2) * n));
        if (!split_ntt) { dc.tabs[m] = tb; continue; }
        // split transform: table 2 m + h for half h; ninv / ninv_q carry the first stage's twiddle psi^brv(1)
        tb.ninv = t.fwd[1];
        tb.ninv_q = t.fwd_q[1];
        for (size_t h = 0; h < 2; h++) {
            // forward twiddles of the two half transforms: stage s of half h is stage s + 1 of the big transform,
            // blocks h 2^s ..: W_h[2^s + b] = W[2^(s+1) + h 2^s + b]
            const size_t at = halves + ((size_t)m * 2 + h) * (n / 2);
            TwPair *dst = tw.data() + at;
            dst[0] = TwPair{ 0, 0 };
            for (size_t m2 = 1; m2 < n / 2; m2 <<= 1)
                for (size_t b = 0; b < m2; b++) {
                    const size_t from = 2 * m2 + h * m2 + b;
                    dst[m2 + b] = TwPair{ t.fwd[from], t.fwd_q[from] };
                }
            tb.fwd = table_ref<TwPair>(at);
            dc.tabs[(size_t)m * 2 + h] = tb;
        }
    }
}

static void build_level(const HeParams &hp, int c, DevLevel &d)
{
    const LevelConstants &h = hp.level[c];
    const u64 mt = (u64)1 << 32;
    std::memset(&d, 0, sizeof(d));
    const int L = h.L, nB = h.nB, nBsk = nB + 1;
    if (L > DMAXL || nBsk > DMAXB) throw std::invalid_argument("too many RNS limbs");
    d.L = L; d.nB = nB; d.nBsk = nBsk; d.E = L + nBsk;
    std::vector<u64> bsk = h.B;
    bsk.push_back(h.m_sk);
    d.t = hp.t;
    d.q_mod_t = h.q_mod_t;
    d.threshold = h.upper_half_threshold;
    d.half = h.q[L - 1] >> 1;
    for (int j = 0; j < L; j++) {
        const u64 qj = h.q[j];
        ModulusInfo mj(qj);
        d.q[j] = make_mod(qj);
        d.ext[j] = d.q[j];
        {
            const int sh = mac_shift_of(qj);                       // both operand halves < 2^sh (sh <= 30); the chunk rules: mac_core.h
            d.mac_shift[j] = (u32)sh;
            d.mac_chunk[j] = mac_chunk_of(qj);
            d.mac_chunk_k[j] = mac_chunk_k_of(qj);                  // (below 7 terms: not used, mac_kara_usable)
            // packed row width (the geometry is there in every context: images of either format load anywhere)
            const u32 w = hp.using_keyswitching ? packed_row_bits(qj) : 64;
            d.mac_bits[j] = w;
            d.mac_row_off[j] = j ? d.mac_row_off[j - 1] + (u32)(hp.n * d.mac_bits[j - 1] / 8) : 0;
            d.mac_mask_hi[j] = mac_mask_hi_of(w, sh);
        }
        d.coeff_div_plain[j] = h.coeff_div_plain[j];
        d.incr[j] = h.upper_half_incr[j];
        d.half_mod[j] = d.half % qj;
        if (j + 1 < L) d.inv_q_last[j] = shoup_const(h.inv_q_last[j], qj);
        d.ext_scale[j] = shoup_const(mj.mul(mt % qj, h.inv_punct_q[j]), qj);
        d.q_to_mt[j] = (u32)h.q_to_mtilde[j];
        d.t_inv_punct_q[j] = shoup_const(mj.mul(hp.t % qj, h.inv_punct_q[j]), qj);
        d.prod_B_q[j] = h.prod_B_mod_q[j];
        d.neg_prod_B_q[j] = (qj - h.prod_B_mod_q[j]) % qj;
        d.s_prod_B_q[j] = shoup_const(d.prod_B_q[j], qj);
        d.s_neg_prod_B_q[j] = shoup_const(d.neg_prod_B_q[j], qj);
        for (int i = 0; i < nB; i++) { d.B_to_q[j][i] = h.B_to_q[j][i]; d.s_B_to_q[j][i] = shoup_const(h.B_to_q[j][i], qj); }
    }
    d.neg_inv_q_mt = (u32)h.neg_inv_q_mod_mtilde;
    for (int i = 0; i < nBsk; i++) {
        const u64 m = bsk[i];
        const ModulusInfo mi(m);
        d.bsk[i] = make_mod(m);
        d.ext[L + i] = d.bsk[i];
        for (int j = 0; j < L; j++) { d.q_to_bsk[i][j] = h.q_to_bsk[i][j]; d.s_q_to_bsk[i][j] = shoup_const(h.q_to_bsk[i][j], m); }
        d.prod_q_bsk[i] = h.prod_q_mod_bsk[i];
        d.s_prod_q_bsk[i] = shoup_const(h.prod_q_mod_bsk[i], m);
        d.s_fl[i] = shoup_const(i < nB ? mi.mul(h.inv_prod_q_mod_bsk[i], h.inv_punct_B[i]) : h.inv_prod_q_mod_bsk[i], m);
        d.inv_mt_bsk[i] = shoup_const(h.inv_mtilde_mod_bsk[i], m);
        for (int j = 0; j < L; j++) d.s_q_to_bsk_mt[i][j] = shoup_const(mi.mul(h.q_to_bsk[i][j] % m, h.inv_mtilde_mod_bsk[i]), m);
        d.s_prod_q_bsk_mt[i] = shoup_const(mi.mul(h.prod_q_mod_bsk[i], h.inv_mtilde_mod_bsk[i]), m);
        d.t_bsk[i] = shoup_const(hp.t % m, m);
        d.inv_prod_q_bsk[i] = shoup_const(h.inv_prod_q_mod_bsk[i], m);
        if (i < nB) {
            d.inv_punct_B[i] = shoup_const(h.inv_punct_B[i], m);
            d.B_to_msk[i] = h.B_to_msk[i];
            d.s_B_to_msk[i] = shoup_const(h.B_to_msk[i], h.m_sk);
        }
    }
    d.inv_prod_B_msk = shoup_const(h.inv_prod_B_mod_msk, h.m_sk);
    d.msk_half = h.m_sk >> 1;
}

// cst * scale[k] of modulus `id` for every position k: a constant with the inverse transform's twist n^-1 psi^-k folded in
static void push_twisted(const HeParams &hp, int id, u64 cst, std::vector<ShoupConst> &out)
{
    const NttTablesHost &tb = hp.ntt[id];
    for (size_t k = 0; k < hp.n; k++) out.push_back(shoup_const(tb.mod.mul(cst, tb.scale[k]), tb.mod.value));
}
// the plain twist of modulus `id` is the transform's own scale table (same {w, wq} layout)
static const ShoupConst *scale_ref(const HeParams &hp, int id) { return table_ref<ShoupConst>(((size_t)id * 3 + 2) * hp.n); }

static void build_levels(const HeParams &hp, DeviceConstants &dc)
{
    const int nl = hp.first_chain_idx + 1;
    dc.levels.resize(nl);
    dc.map_ext.assign((size_t)nl * DMAXE, 0);
    dc.map_ks.assign((size_t)nl * (DMAXL + 1) * DMAXL, 0);
    dc.map_ksacc.assign((size_t)nl * (DMAXL + 1), 0);
    for (int c = 0; c < nl; c++) {
        DevLevel &d = dc.levels[c];
        build_level(hp, c, d);
        const int L = d.L;
        for (int j = 0; j < L; j++) dc.map_ext[(size_t)c * DMAXE + j] = j;
        for (int i = 0; i < d.nBsk; i++) dc.map_ext[(size_t)c * DMAXE + L + i] = hp.bsk_id(d.nB, i);
        // key-switch maps
        for (int I = 0; I <= L; I++) {
            const int id = I == L ? hp.K - 1 : I;
            for (int J = 0; J < L; J++) dc.map_ks[(size_t)c * (DMAXL + 1) * DMAXL + (size_t)I * L + J] = id;
            dc.map_ksacc[(size_t)c * (DMAXL + 1) + I] = id;
        }
    }
    // per-position constants of the unrolled finish kernels: their own constant times the inverse transform's twist
    // (fin_q / fin_b), and the matching inverse-NTT maps
    dc.map_ext_fin = dc.map_ext;
    for (int c = 0; c < nl; c++) {
        DevLevel &d = dc.levels[c];
        if (!behz_unrolled(d.L, d.nB)) continue;
        for (int e = 0; e < d.E; e++) {
            (e < d.L ? d.fin_q[e] : d.fin_b[e - d.L]) = table_ref<ShoupConst>(dc.fin.size());
            push_twisted(hp, dc.map_ext[(size_t)c * DMAXE + e], e < d.L ? d.t_inv_punct_q[e].w : d.t_bsk[e - d.L].w, dc.fin);
            dc.map_ext_fin[(size_t)c * DMAXE + e] |= NTT_MAP_RAW;
        }
    }
    // per-position constants of the drop-last-limb consumers of a RAW inverse transform (drop_tw / last_tw)
    for (int c = 1; c < nl; c++) {
        DevLevel &d = dc.levels[c];
        for (int j = 0; j + 1 < d.L; j++) {
            d.drop_tw[j] = table_ref<ShoupConst>(dc.drop.size());
            push_twisted(hp, j, d.inv_q_last[j].w, dc.drop);
        }
        d.last_tw = scale_ref(hp, d.L - 1);
    }
    dc.map_ksacc_raw = dc.map_ksacc;
    for (int &v : dc.map_ksacc_raw) v |= NTT_MAP_RAW;
    dc.map_ct.resize(DMAXL + DMAXB + 4);                          // identity over every modulus id (incl. plain modulus)
    for (size_t i = 0; i < dc.map_ct.size(); i++) dc.map_ct[i] = (int)i;
}

// key-switching constants
static void build_key(const HeParams &hp, DeviceConstants &dc)
{
    DevKey &k = dc.key;
    std::memset(&k, 0, sizeof(k));
    k.K = hp.K;
    for (int j = 0; j < hp.K; j++) k.q[j] = make_mod(hp.key_q[j]);
    if (hp.K > 1) {
        const u64 p = hp.key_q[hp.K - 1];
        k.p_half = p >> 1;
        for (int j = 0; j < hp.K - 1; j++) {
            k.p_half_mod[j] = k.p_half % hp.key_q[j];
            k.inv_p[j] = shoup_const(hp.inv_p_mod_q[j], hp.key_q[j]);
            // per-position constants of the mod-down behind a RAW inverse transform (md_tw / p_tw)
            k.md_tw[j] = table_ref<ShoupConst>(dc.mdtw.size());
            push_twisted(hp, j, hp.inv_p_mod_q[j], dc.mdtw);
        }
        k.p_tw = scale_ref(hp, hp.K - 1);
    }
    // seed expansion (Engine::queue_seed_expand): the key level is a data level only without key switching
    if (hp.K - 1 > hp.first_chain_idx && hp.K <= DMAXL) {
        dc.key_level.resize(1);
        DevLevel &d = dc.key_level[0];
        std::memset(&d, 0, sizeof(d));
        d.L = hp.K;
        for (int j = 0; j < hp.K; j++) d.q[j] = k.q[j];
    }
    for (u64 q : hp.key_q) {
        dc.max_multiple.push_back(~(u64)0 - (~(u64)0 % q) - 1);    // util/rlwe.cpp: max_multiple
        dc.row_bits.push_back(packed_row_bits(q));
    }
}

DeviceConstants build_device_constants(const HeParams &hp)
{
    DeviceConstants dc;
    build_transform_tables(hp, dc);
    build_levels(hp, dc);
    build_key(hp, dc);
    dc.data_primes_narrow = true;
    for (u64 q : hp.key_q) dc.data_primes_narrow = dc.data_primes_narrow && ntt_is_narrow(q, hp.logn);
    // launches over the extended base (map_ext / map_ext_fin) state narrowness with this flag: with the engine's own auxiliary base
    // (params.cpp, narrow_aux_base) the largest forward launch of a query, the extension transform, takes the 8-wave form
    dc.ext_primes_narrow = dc.data_primes_narrow;
    for (u64 m : hp.aux_primes) dc.ext_primes_narrow = dc.ext_primes_narrow && ntt_is_narrow(m, hp.logn);
    // update_bundle's decode (bin_update.h: bin_unlift) refuses otherwise
    dc.unlift_exact = hp.batching && hp.key_q[0] / 2 >= hp.t && hp.key_q[0] > 2 * hp.t;
    return dc;
}

EngineSwitches read_switches()
{
    EngineSwitches s;
    auto flag = [](const char *name, auto &out) { if (const char *v = std::getenv(name)) out = std::atoi(v) != 0; };
    auto size = [](const char *name, size_t &out) { if (const char *v = std::getenv(name)) out = std::strtoull(v, nullptr, 10); };
    flag("APSU_HE_SPLIT", s.two_stream_default);
    flag("APSU_HE_MAC_KARA", s.mac_kara);
    flag("APSU_HE_EVAL_SIDE", s.eval_side);
    flag("APSU_HE_PACKED_ROWS", s.packed_rows);
    flag("APSU_HE_EVAL_PER_TERM", s.force_per_term);
    flag("APSU_HE_SEED_EXPAND_HOST", s.seed_expand_host);
    flag("APSU_HE_FUSE_TAIL", s.fuse_tail);
    size("APSU_HE_EVAL_WS_BYTES", s.eval_ws_bytes);
    size("APSU_HE_ARENA_BYTES", s.arena_bytes);
    size("APSU_HE_NTT_LATENCY_LIMBS", s.ntt_latency_limbs);
    size("APSU_HE_SEED_REJ_CAP", s.seed_rej_cap);
    return s;
}

} // namespace apsu_he
