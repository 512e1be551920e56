// Querier side (N5): the pure device functions of key generation and query encryption -- where every random draw sits in the
// generator's output, the word -> value maps of the two samplers, and the exponentiation of PlaintextPowers
// (sender/apsu/plaintext_powers.cpp:51-99).  __host__ __device__, so that the CPU test tier runs the same code against Python
// (emu/query.cpp: emu_qs_*).
//
// One generator per call: SEAL's Blake2xb generator (blake2x.h) under the caller's 64-byte seed, u[0], u[1], ... its 32-bit
// outputs.  A 64-byte stream block holds 16 of them; a 64-bit draw is w = u[p] + 2^32 u[p + 1] at an even position p, i.e. one
// of the eight little-endian words of a block.  The stream is cut into three disjoint ranges of blocks:
//   secret      blocks [0, QS_POLY_BLOCKS):                coefficient k of s draws word k (p = 2k)
//   public seed block  QS_SEED_BLOCK0 + o:                 the eight words of the block are object o's prng_seed_type
//   noise       blocks QS_NOISE_BLOCK0 + o QS_POLY_BLOCKS + [0, QS_POLY_BLOCKS):   coefficient k of object o's e draws word k of its range
// Objects: o = i for relinearisation key i (i < QS_KEY_OBJECTS), o = QS_KEY_OBJECTS + c for ciphertext c of a query.
// The public seeds are outputs of the secret stream; nothing is ever drawn from a public seed but the public polynomial.
#pragma once
#include "modmath.h"

namespace apsu_he {

constexpr u64 QS_MAX_N = 32768;                                   // largest poly_modulus_degree
constexpr u64 QS_POLY_BLOCKS = QS_MAX_N / 8;                      // stream blocks of one polynomial's draws (one word per coefficient)
constexpr u64 QS_KEY_OBJECTS = 16;                                // objects reserved for relinearisation keys (K - 1 <= 8 are used)
constexpr u64 QS_MAX_OBJECTS = (u64)1 << 20;                      // objects of one seed; a query has at most QS_MAX_OBJECTS - QS_KEY_OBJECTS ciphertexts
constexpr u64 QS_SECRET_BLOCK0 = 0;
constexpr u64 QS_SEED_BLOCK0 = QS_POLY_BLOCKS;
constexpr u64 QS_NOISE_BLOCK0 = (u64)1 << 21;
static_assert(QS_SECRET_BLOCK0 + QS_POLY_BLOCKS <= QS_SEED_BLOCK0 && QS_SEED_BLOCK0 + QS_MAX_OBJECTS <= QS_NOISE_BLOCK0, "stream ranges overlap");

HD u64 qs_secret_block(u64 k) { return QS_SECRET_BLOCK0 + (k >> 3); }
HD u64 qs_seed_block(u64 object) { return QS_SEED_BLOCK0 + object; }
HD u64 qs_noise_block(u64 object, u64 k) { return QS_NOISE_BLOCK0 + object * QS_POLY_BLOCKS + (k >> 3); }

// uniform over {-1, 0, 1}: floor(3 w / 2^64) - 1; the three values' probabilities differ by at most 2^-64
HD int qs_ternary(u64 w) { return (int)mulhi64(w, 3) - 1; }
// SEAL's centred binomial noise (util/rlwe.cpp sample_poly_cbd: 21 coin pairs, |e| <= 21, variance 10.5): bits 0..20 minus bits 21..41
HD int qs_cbd(u64 w) { return __builtin_popcountll(w & 0x1FFFFF) - __builtin_popcountll((w >> 21) & 0x1FFFFF); }
// a small signed value as a residue of q
HD u64 qs_residue(int v, u64 q) { return v < 0 ? q - (u64)(-v) : (u64)v; }

// x^e mod t, x < t (square and multiply from the top bit; e = 0 gives 1)
HD u64 qs_pow_mod(u64 x, u32 e, const Mod &t)
{
    u64 r = 1 % t.q;
    for (int b = 31 - (e ? __builtin_clz(e) : 31); b >= 0; b--) {
        r = mulmod(r, r, t);
        if ((e >> b) & 1) r = mulmod(r, x, t);
    }
    return r;
}

// The rounding of the querier's decryption (k_decrypt_round, k_decrypt_round_budget): round(t x / q0) mod t for x < q0 < 2^62,
// 2 <= t < 2^61; rem receives (t x + floor(q0 / 2)) mod q0
HD u64 decrypt_round_coeff(u64 x, u64 q0, u64 t, u64 &rem)
{
    u128p num = mul128(x, t);
    add128(num, u128p{ q0 >> 1, 0 });
    // floor(num / q0) mod t by restoring division, the quotient folded mod t on the fly (num < 2^124)
    u64 quo = 0;
    rem = 0;
    for (int i = 127; i >= 0; i--) {
        const u64 bit = i >= 64 ? (num.hi >> (i - 64)) & 1 : (num.lo >> i) & 1;
        rem = (rem << 1) | bit;                                   // rem < q0 < 2^62 before the shift
        quo <<= 1;                                                // quo < t < 2^61
        if (rem >= q0) { rem -= q0; quo |= 1; }
        if (quo >= t) quo -= t;
    }
    return quo;
}

} // namespace apsu_he
