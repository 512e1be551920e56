// CPU emulation, the querier's side and the Blake2xb streams (query_side.h, blake2x.h).  Model: tests/query_side_model.py.
#include "emu_common.h"
#include "blake2x.h"
#include "params.h"
#include "query_side.h"

using namespace apsu_he;

extern "C" {

// `count` 32-bit outputs of the Blake2xb generator (blake2x.h, the code k_fill_blake2xb runs) starting at output `first`
int emu_blake2xb_values(const uint64_t *seed, uint64_t first, uint32_t *out, int count)
{
    Blake2xbSeed sd;
    for (int i = 0; i < 8; i++) sd.w[i] = seed[i];
    u64 blk[8];
    u64 have = ~(u64)0;
    for (int i = 0; i < count; i++) {
        const u64 g = first + (u64)i;
        if (g / 16 != have) { have = g / 16; blake2xb_stream_block(sd, have, blk); }
        out[i] = blake2xb_stream_u32(blk, (unsigned)(g % 16));
    }
    return 0;
}

// N5 (query_side.h, the functions k_sample_ternary / k_sample_cbd / k_plain_powers run): the secret's n coefficients under `seed`
int emu_qs_secret(const uint64_t *seed, uint64_t n, int8_t *out)
{
    Blake2xbSeed sd;
    for (int i = 0; i < 8; i++) sd.w[i] = seed[i];
    u64 blk[8];
    for (u64 k = 0; k < n; k++) {
        if (k % 8 == 0) blake2xb_stream_block(sd, qs_secret_block(k), blk);
        out[k] = (int8_t)qs_ternary(blk[k % 8]);
    }
    return 0;
}
// the noise polynomial of `object`
int emu_qs_noise(const uint64_t *seed, uint64_t object, uint64_t n, int8_t *out)
{
    Blake2xbSeed sd;
    for (int i = 0; i < 8; i++) sd.w[i] = seed[i];
    u64 blk[8];
    for (u64 k = 0; k < n; k++) {
        if (k % 8 == 0) blake2xb_stream_block(sd, qs_noise_block(object, k), blk);
        out[k] = (int8_t)qs_cbd(blk[k % 8]);
    }
    return 0;
}
// the public seed of `object` (eight words)
int emu_qs_public_seed(const uint64_t *seed, uint64_t object, uint64_t *out)
{
    Blake2xbSeed sd;
    for (int i = 0; i < 8; i++) sd.w[i] = seed[i];
    blake2xb_stream_block(sd, qs_seed_block(object), out);
    return 0;
}
// the layout's constants: max n, blocks per polynomial, key objects, max objects, first block of the secret / seed / noise ranges
int emu_qs_layout(uint64_t *out, int cap)
{
    const u64 v[7] = { QS_MAX_N, QS_POLY_BLOCKS, QS_KEY_OBJECTS, QS_MAX_OBJECTS, QS_SECRET_BLOCK0, QS_SEED_BLOCK0, QS_NOISE_BLOCK0 };
    for (int i = 0; i < 7 && i < cap; i++) out[i] = v[i];
    return 7;
}
// first stream block of coefficient k's draw: kind 0 secret, 1 public seed of `object`, 2 noise of `object`
uint64_t emu_qs_block(int kind, uint64_t object, uint64_t k)
{
    return kind == 0 ? qs_secret_block(k) : kind == 1 ? qs_seed_block(object) : qs_noise_block(object, k);
}
int emu_qs_pow_mod(uint64_t t, const uint64_t *x, const uint32_t *e, uint64_t *out, int count)
{
    ModulusInfo mi(t);
    const Mod m{ t, mi.ratio[0], mi.ratio[1] };
    for (int i = 0; i < count; i++) out[i] = qs_pow_mod(x[i], e[i], m);
    return 0;
}
// decrypt_round_coeff (the code k_decrypt_round and k_decrypt_round_budget run) on `count` values x < q0: out = round(t x / q0) mod t,
// rem = (t x + floor(q0 / 2)) mod q0.  -1 for what the kernels' range argument does not cover (q0 >= 2^62, t >= 2^61, t < 2, t >= q0, x >= q0).
int emu_qs_decrypt_round(uint64_t q0, uint64_t t, const uint64_t *x, uint64_t *out, uint64_t *rem, int count)
{
    if (q0 >> 62 || t >> 61 || t < 2 || t >= q0) return -1;
    for (int i = 0; i < count; i++) if (x[i] >= q0) return -1;
    for (int i = 0; i < count; i++) out[i] = decrypt_round_coeff(x[i], q0, t, rem[i]);
    return 0;
}

} // extern "C"
