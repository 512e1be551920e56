// Constant blocks of the query-evaluation engine: the plain-old-data structs the kernels read through wave-uniform (scalar) loads,
// and the ONE host function that derives every one of them from HeParams (build_device_constants, dev_consts.cpp).
// No HIP here: the same code is part of the engine library and of the CPU emulation library, so the no-GPU tests see every
// value a context uploads (tests/test_dev_consts_cpu.py).
#pragma once
#include <cstddef>
#include <vector>

#include "modmath.h"
#include "ntt_core.h"
#include "ntt_form.h"
#include "params.h"

namespace apsu_he {

constexpr int EW_T = 256;           // threads per workgroup of the coefficient-parallel kernels
constexpr int DMAXL = 8;            // limbs of q at a data level
constexpr int DMAXB = DMAXL + 2;    // |Bsk|
constexpr int DMAXE = DMAXL + DMAXB; // limbs of an extended (q u Bsk) polynomial
constexpr u32 SEED_REJ_CAP = 8192;  // rejected positions per object that the seed expansion's fix-up pass can hold (kernels_ew.hip: k_seed_fix)

struct ShoupConst { u64 w, wq; };

// One level of the modulus chain (chain_idx = L-1).
struct DevLevel {
    int L, nB, nBsk, E;                         // E = L + nBsk limbs of an extended polynomial
    Mod q[DMAXL];
    Mod bsk[DMAXB];                             // B_0..B_{nB-1}, m_sk
    Mod ext[DMAXE];                             // q_0..q_{L-1}, Bsk..   (modulus of each ext limb)
    u64 t;
    u32 mac_shift[DMAXL], mac_chunk[DMAXL];     // k_mac: operand split width s = ceil(bits(q_j)/2) and terms per carry-free chunk
    u32 mac_chunk_k[DMAXL];                     // ... of the three-product form (middle products have 2 s + 2 bits)
    // Bit-packed database rows (round 4; k_mac<.., PACKED>): limb j of a stored NTT-form plaintext takes mac_bits[j] bits per
    // coefficient -- the smallest width >= bits(q_j) for which a lane's 16-byte window covers its two coefficients at every
    // position (48, 49, 50, 52, 56; else 64 = not packed) -- in rows of n * mac_bits[j] / 8 bytes at byte offset mac_row_off[j]
    // inside a plaintext slot.  Rows depend on the limb only, so every level's prefix of them is the same.
    u32 mac_bits[DMAXL], mac_row_off[DMAXL], mac_mask_hi[DMAXL];
    // add_plain (App. B7) and plaintext lift (B5)
    u64 coeff_div_plain[DMAXL];
    u64 q_mod_t, threshold;
    u64 incr[DMAXL];
    // drop-last-limb with rounding (B8)
    u64 half;
    u64 half_mod[DMAXL];
    ShoupConst inv_q_last[DMAXL];
    // BEHZ extension: fastbconv_m_tilde + sm_mrq (B9 steps 1-2)
    ShoupConst ext_scale[DMAXL];                // m_tilde * (Q/q_j)^-1 mod q_j
    u64 q_to_bsk[DMAXB][DMAXL];                 // (Q/q_j) mod Bsk_i
    u32 q_to_mt[DMAXL];                         // (Q/q_j) mod 2^32
    u32 neg_inv_q_mt;
    u64 prod_q_bsk[DMAXB];
    ShoupConst inv_mt_bsk[DMAXB];
    // BEHZ finish: multiply by t, fast_floor, fastbconv_sk (B9 steps 6-8)
    ShoupConst t_inv_punct_q[DMAXL];            // t * (Q/q_j)^-1 mod q_j
    ShoupConst t_bsk[DMAXB];                    // t mod Bsk_i
    ShoupConst inv_prod_q_bsk[DMAXB];
    ShoupConst inv_punct_B[DMAXB];
    u64 B_to_q[DMAXL][DMAXB];                   // (B/b_i) mod q_j
    u64 B_to_msk[DMAXB];
    ShoupConst inv_prod_B_msk;
    u64 prod_B_q[DMAXL], neg_prod_B_q[DMAXL];
    u64 msk_half;
    // the same matrices as Shoup constants for the fully unrolled kernels (L = nB <= 3): every product is a
    // lazy Shoup product (< 2m), sums stay below 8m < 2^64 and are reduced once
    ShoupConst s_q_to_bsk[DMAXB][DMAXL];
    ShoupConst s_prod_q_bsk[DMAXB];
    // the same two with m_tilde^-1 folded in (sm_mrq's closing product becomes a plain reduction: behz_ext2_body)
    ShoupConst s_q_to_bsk_mt[DMAXB][DMAXL];
    ShoupConst s_prod_q_bsk_mt[DMAXB];
    ShoupConst s_fl[DMAXB];                     // i < nB: (Q^-1 * (B/b_i)^-1) mod b_i ; i = nB: Q^-1 mod m_sk
    ShoupConst s_B_to_q[DMAXL][DMAXB];
    ShoupConst s_B_to_msk[DMAXB];
    ShoupConst s_prod_B_q[DMAXL], s_neg_prod_B_q[DMAXL];
    // The unrolled finish kernels (L = nB <= 3) consume the output of an inverse NTT and start by multiplying it with a
    // constant (t (Q/q_j)^-1 for the q limbs, t for the Bsk limbs).  For them the inverse transform leaves out its own final
    // twist (n^-1 psi^-k, one exact Shoup product per coefficient) and writes the raw lazy value; the twist rides on the
    // finish's constant instead: fin_q[j][k] = t (Q/q_j)^-1 n^-1 psi_j^-k mod q_j, fin_b[i][k] = t n^-1 psi_i^-k mod Bsk_i.
    // Same residues, one modular product per coefficient less.  Null for levels that use the generic finish.
    const ShoupConst *fin_q[DMAXL];
    const ShoupConst *fin_b[DMAXB];
    // The same idea for the consumers of an inverse NTT that drop this level's last limb (mod_switch_to_next: the fused
    // drop + extension of eval_patstock's inner polynomials, the i = 0 block's finish): the transform writes raw values and
    // the twist rides on the drop's own constant, drop_tw[j][k] = n^-1 psi_j^-k q_last^-1 mod q_j (j < L - 1);
    // last_tw[k] = n^-1 psi_{L-1}^-k (the dropped limb needs its canonical residue).  Null where unused.
    const ShoupConst *drop_tw[DMAXL];
    const ShoupConst *last_tw;
};

// Key-switching constants (App. B10); moduli indexed by key limb.
struct DevKey {
    int K;
    Mod q[DMAXL + 1];
    u64 p_half;
    u64 p_half_mod[DMAXL];
    ShoupConst inv_p[DMAXL];
    // mod-down behind a RAW inverse transform: md_tw[j][k] = n^-1 psi_j^-k p^-1 mod q_j, p_tw[k] = n^-1 psi_p^-k mod p
    const ShoupConst *md_tw[DMAXL];
    const ShoupConst *p_tw;
};

// Limb -> modulus maps of the transform launches (device.h: launch_ntt).  An inverse transform of a limb whose map entry carries
// NTT_MAP_RAW writes its result WITHOUT the final twist n^-1 psi^-k and without the final reduction.
constexpr int NTT_MAP_RAW = 1 << 30, NTT_MAP_MASK = NTT_MAP_RAW - 1;

inline ShoupConst shoup_const(u64 w, u64 q) { return ShoupConst{ w, (u64)(((u128)w << 64) / q) }; }
inline Mod make_mod(u64 q) { ModulusInfo m(q); return Mod{ q, m.ratio[0], m.ratio[1] }; }
// width of a bit-packed database row of a prime (DevLevel::mac_bits): the smallest w >= max(bits, 32) whose 2-coefficient group fits a
// lane's 16-byte window at every position: the group starts at bit 2 w m, i.e. (2 w m) mod 32 <= 32 - gcd(2 w, 32) into its first dword
uint32_t packed_row_bits(u64 q);

// The per-modulus table of the transforms.  logn: the stages that run inside one workgroup (narrowness is a property of the modulus
// AND that depth).  The first form carries what follows from the modulus alone (reductions, range control); the second adds n^-1 and
// the twiddle tables, given wherever they live (host arrays for the emulation, device addresses or table references for the engine).
// (inline: params.cpp chooses the auxiliary base with it and stays linkable on its own)
inline NttTable make_ntt_table(u64 q, int logn)
{
    const ModulusInfo m(q);
    NttTable tb{};
    tb.q = q;
    tb.r1 = m.ratio[1];
    tb.r0 = m.ratio[0];
    tb.narrow = ntt_is_narrow(q, logn) ? 1 : 0;
    ntt_fold_params(q, tb.fold_k, tb.fold_c);
    tb.wide_d4 = ntt_wide_d4(q, tb.narrow != 0);
    return tb;
}
inline NttTable make_ntt_table(const NttTablesHost &t, int logn, const TwPair *fwd, const TwPair *dit, const TwPair *scale)
{
    NttTable tb = make_ntt_table(t.mod.value, logn);
    tb.ninv = t.ninv;
    tb.ninv_q = t.ninv_q;
    tb.fwd = fwd;
    tb.dit = dit;
    tb.scale = scale;
    return tb;
}

// Everything a context uploads once, as host vectors.  A pointer member of a struct in here (NttTable::fwd / dit / scale,
// DevLevel::fin_q / fin_b / drop_tw / last_tw, DevKey::md_tw / p_tw) holds a TABLE REFERENCE until relocate(): 1 + the element offset
// into the table it points into (16-byte elements; 0 stays null).  Which table: fwd / dit / scale / last_tw / p_tw -> tw,
// fin_q / fin_b -> fin, drop_tw -> drop, md_tw -> mdtw.
struct DeviceConstants {
    std::vector<TwPair> tw;             // per modulus [fwd n][dit n][scale n]; at logn 15 then per modulus the two halves' forward tables [n/2][n/2]
    std::vector<NttTable> tabs;         // per modulus (logn 15: per modulus and half)
    std::vector<ShoupConst> fin, drop, mdtw;
    std::vector<DevLevel> levels;       // chain_idx 0 .. first_chain_idx
    DevKey key;
    std::vector<int> map_ext, map_ext_fin, map_ks, map_ksacc, map_ksacc_raw, map_ct;
    // seed expansion at the key level where that is no data level (K - 1 > first_chain_idx): a DevLevel-shaped view that carries the
    // key moduli only (empty otherwise, or with more key limbs than a DevLevel holds); max_multiple (util/rlwe.cpp) per key prime
    std::vector<DevLevel> key_level;
    std::vector<u64> max_multiple;
    bool data_primes_narrow = false;    // every key prime runs the transform without range control (ntt_is_narrow)
    bool ext_primes_narrow = false;     // ... and so does every modulus of the extended base q u Bsk (HeParams::aux_narrow)
    bool unlift_exact = false;          // q_0 > 2 t: a stored residue tells its value mod t (bin_update.h: bin_unlift)
    std::vector<u32> row_bits;          // packed_row_bits per key prime
    // table references -> addresses, once the tables have theirs (a table nothing refers to may be null)
    void relocate(const TwPair *tw_base, const ShoupConst *fin_base, const ShoupConst *drop_base, const ShoupConst *mdtw_base);
};
// throws std::invalid_argument for a ring size without a transform plan or more limbs than the blocks hold
DeviceConstants build_device_constants(const HeParams &hp);

// Environment switches, read once per context.  Round 5 retired the switches of A/B experiments that were decided in earlier rounds
// together with their losing code paths (the records are in profiles/r03_ab_*.txt and profiles/r04_ab_*.txt).  What is left either
// selects a data format, sizes a buffer, or forces a correctness fallback that the engine otherwise takes by itself.  A variable that
// is set counts as on when atoi(value) != 0.  (APSU_HE_AUX_BASE=seal, SEAL's 61-bit auxiliary BEHZ base instead of the narrow one,
// is read by c_api.cpp: it is needed before HeParams exists.)
struct EngineSwitches {
    static constexpr size_t ARENA_AUTO = ~(size_t)0;
    int two_stream_default = -1;                 // APSU_HE_SPLIT=0/1          default of apsu_he_set_two_stream (profiling scripts: one-stream kernel traces)
    bool eval_side = true;                       // APSU_HE_EVAL_SIDE=0        the evaluation's side work (coefficient-form sums, i = 0 finish) stays on the main stream
    // BinBundle plaintexts bit-packed in HBM (12.5 % fewer bytes for 56-bit primes, 22 % for 50-bit ones; k_mac<.., PACKED>): in-process
    // A/B on 16M-4096 -0.146 +- 0.017 ms (-4.2 %) on the whole query, -2.4 % on the N = 8 shard, same bits
    // (profiles/r04_ab_packed_rows.txt).  Only with key switching (the single-prime paths keep dense rows).
    bool packed_rows = true;                     // APSU_HE_PACKED_ROWS=0      BinBundle rows as dense 64-bit words (images of either format load anywhere)
    size_t eval_ws_bytes = (size_t)6 << 30;      // APSU_HE_EVAL_WS_BYTES=n    evaluation workspace -> BinBundles per chunk (default 6 GiB)
    size_t arena_bytes = ARENA_AUTO;             // APSU_HE_ARENA_BYTES=n      initial workspace arena (grows on demand; default by ring size)
    bool force_per_term = false;                 // APSU_HE_EVAL_PER_TERM=1    eval_patstock's products finished one by one (the fallback of the summed finish)
    int mac_kara = -1;                           // APSU_HE_MAC_KARA=0/1       three-product k_mac forced off / on (default: by chain length)
    bool seed_expand_host = false;               // APSU_HE_SEED_EXPAND_HOST=1 seeded objects expanded by the host codec (the fallback of the device sampler)
    // (values outside 1 .. SEED_REJ_CAP are refused at create; the compiled list stride and LDS array stay SEED_REJ_CAP)
    size_t seed_rej_cap = SEED_REJ_CAP;          // APSU_HE_SEED_REJ_CAP=n     rejected words per seeded object the device list takes before the host redoes the object (tests: the fallback at small sizes)
    bool fuse_tail = true;                       // APSU_HE_FUSE_TAIL=0        eval_patstock's last mod-down as its own launch instead of inside the epilogue kernel (round 6)
    // The latency form of the LDS-resident transform (ntt_core.h plan_k, c = 8): a limb's workgroup has twice the waves, so a launch
    // that gives a CU at most one limb hides that limb's LDS turnarounds and table loads behind three other waves per SIMD.
    // Crossovers: ntt_form.h, ntt_form (tools/microbench/ntt_forms.hip, profiles/r06_ntt_forms_n8192.txt / _n4096.txt).
    size_t ntt_latency_limbs = NTT_FORM_AUTO;    // APSU_HE_NTT_LATENCY_LIMBS=n transform launches of at most n limbs take the latency form (8 coefficients per
                                                 //                            lane; round 6); 0 = always the throughput form.  Default: the measured crossover
};
EngineSwitches read_switches();

} // namespace apsu_he
