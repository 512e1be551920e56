// Cuckoo hashing (N1, both parties): where an item goes, the querier's table, and the database side's grouping by location.
// Pure functions shared by the kernels (kernels_cuckoo.hip), the engine's host steps and the CPU test tier (emu/cuckoo.cpp); an
// independent Python model is tests/cuckoo_model.py.  Contracts: include/apsu_he.h (apsu_he_item_locations, apsu_he_cuckoo_table).
//
// The location function is Kuku 2.x's LocFunc, restated from memory [Kuku-recall] and UNPINNED, like the SEAL object layer: no Kuku
// source and no known-answer vector has been held against it.
//   item_type = 16 bytes, location_type = uint32.  Function f's seed is make_item(f, 0): f as 8 little-endian bytes, then 8 zero bytes.
//   tab_f[16][256] (uint32) = the 16384 bytes of blake2xb(out = 16384, in = the 16 seed bytes, no key), little-endian words: root hash
//   under the parameter block {digest 64, key 0, fanout 1, depth 1, xof_length 16384}, then 256 expansion nodes as in blake2x.h.
//   loc_f(item) = (tab_f[0][item[0]] ^ tab_f[1][item[1]] ^ ... ^ tab_f[15][item[15]]) % table_size,   f < hash_func_count.
//
// The table rule is the engine's own (the reference inserts sequentially with a random walk under its own generator; the protocol needs
// only that every item sits at one of its own locations).  Item i starts with function index h_i = 0, active.  Round r < max_rounds:
//   propose: every active item does a 64-bit min on slot[loc_{h_i}(i)] with the key ((max_rounds - 1 - r) << 32) | i; an empty slot
//            holds ~0, so a newer round beats any older occupant and within a round the lowest index wins, in whatever order.
//   settle:  (behind a barrier) every item that is not a duplicate reads its slot: its own key -> placed; a winner whose 16 bytes
//            equal its own -> DUPLICATE of the winner for good (equal items move in lockstep until the lowest index of them wins, so
//            that one survives); otherwise h_i = (h_i + 1) % hash_func_count and it is active again.
// Done when no item is active; an item still active after max_rounds is a failure and no table is returned.
#pragma once
#include <stddef.h>
#include "blake2x.h"

namespace apsu_he {

constexpr u32 CUCKOO_MAX_FUNCS = 8;                       // params.cpp bounds hash_func_count to 1..8
constexpr u32 CUCKOO_TAB_WORDS = 16 * 256;                // one function's tables: tab[pos][byte], 16 KiB
constexpr u32 CUCKOO_TAB_NODES = CUCKOO_TAB_WORDS * 4 / 64;   // 256 expansion nodes of 64 bytes
constexpr u32 CUCKOO_NONE = 0xFFFFFFFFu;                  // no item in a slot; no location for a duplicate
constexpr u64 CUCKOO_EMPTY = ~(u64)0;
constexpr u64 CUCKOO_MAX_ROUNDS = (u64)1 << 32;           // the round has 32 bits of the key
constexpr u32 CUCKOO_DEFAULT_ROUNDS = 500;                // the reference's cuckoo_table_insert_attempts
// k_cuckoo_insert's table in LDS: 64 KiB of static LDS less the two words the workgroup votes with
constexpr u32 CUCKOO_LDS_SLOTS = (65536 - 64) / 8;
constexpr int CUCKOO_INSERT_T = 1024;                     // lanes of the one workgroup
constexpr int CUCKOO_LOC_T = 1024;                        // lanes per workgroup of k_cuckoo_locations
constexpr u32 CUCKOO_LOC_GROUP = 4;                       // at most this many functions staged into LDS at a time (64 KiB)

// root = BLAKE2b-512(the 16 seed bytes of function f) under xof_length 16384
HD void cuckoo_tab_root(u32 f, u64 root[8])
{
    blake2b_init(root, (u64)64 | ((u64)1 << 16) | ((u64)1 << 24), (u64)(CUCKOO_TAB_WORDS * 4) << 32, 0);
    u64 m[16];
#pragma unroll
    for (int i = 0; i < 16; i++) m[i] = 0;
    m[0] = f;
    blake2b_compress(root, m, 16, true);
}

// expansion node `node` < 256: the eight little-endian words of bytes [64 node, 64 node + 64) = tab words [16 node, 16 node + 16)
HD void cuckoo_tab_node(const u64 root[8], u32 node, u64 out[8])
{
    blake2b_init(out, (u64)64 | ((u64)64 << 32), (u64)node | ((u64)(CUCKOO_TAB_WORDS * 4) << 32), (u64)64 << 8);
    u64 m[16];
#pragma unroll
    for (int i = 0; i < 8; i++) { m[i] = root[i]; m[8 + i] = 0; }
    blake2b_compress(out, m, 64, true);
}

// tab[16][256] of function f
inline void cuckoo_tables(u32 f, u32 *tab)
{
    u64 root[8], out[8];
    cuckoo_tab_root(f, root);
    for (u32 node = 0; node < CUCKOO_TAB_NODES; node++) {
        cuckoo_tab_node(root, node, out);
        for (int i = 0; i < 8; i++) { tab[node * 16 + 2 * i] = (u32)out[i]; tab[node * 16 + 2 * i + 1] = (u32)(out[i] >> 32); }
    }
}

// the tabulation hash of an item given as its four little-endian 32-bit words; tab: one function's tables
HD u32 cuckoo_hash(const u32 *tab, u32 w0, u32 w1, u32 w2, u32 w3)
{
    const u32 w[4] = { w0, w1, w2, w3 };
    u32 x = 0;
#pragma unroll
    for (int p = 0; p < 16; p++) x ^= tab[p * 256 + ((w[p >> 2] >> (8 * (p & 3))) & 0xFF)];
    return x;
}
// k_cuckoo_locations' form of the same hash for G = 1, 2 or 4 functions at once.  img: the functions' tables interleaved,
// img[(pos * 256 + byte) * G + g] = tab_g[pos][byte], so that ONE read of G words serves all G functions (cuckoo_group_image).
constexpr u32 cuckoo_group(u32 H) { return H >= 3 ? 4 : H; }            // functions per staged group: 1, 2, 4 (16 KiB of LDS each)
template <int G> struct CuckooWords;
template <> struct CuckooWords<2> { typedef u32 type __attribute__((vector_size(8), __may_alias__)); };
template <> struct CuckooWords<4> { typedef u32 type __attribute__((vector_size(16), __may_alias__)); };
template <int G> HD void cuckoo_hash_group(const u32 *img, u32 w0, u32 w1, u32 w2, u32 w3, u32 x[G])
{
    const u32 w[4] = { w0, w1, w2, w3 };
#pragma unroll
    for (int g = 0; g < G; g++) x[g] = 0;
#pragma unroll
    for (int p = 0; p < 16; p++) {
        const u32 *e = img + (size_t)(p * 256 + ((w[p >> 2] >> (8 * (p & 3))) & 0xFF)) * G;
        if constexpr (G == 1) x[0] ^= e[0];
        else {                                                      // one read of 8 or 16 bytes (ds_read_b64 / ds_read_b128 on the device)
            const typename CuckooWords<G>::type v = *reinterpret_cast<const typename CuckooWords<G>::type *>(e);
#pragma unroll
            for (int g = 0; g < G; g++) x[g] ^= v[g];
        }
    }
}
// word idx < G * CUCKOO_TAB_WORDS of the staging loop: function g0 + idx / CUCKOO_TAB_WORDS, table word idx % CUCKOO_TAB_WORDS (consecutive
// idx read consecutive words of tabs[H][16][256]) -> where it goes in the image; a function >= H has no table and its words are 0
HD u32 cuckoo_group_image(u32 idx, u32 G) { return (idx % CUCKOO_TAB_WORDS) * G + idx / CUCKOO_TAB_WORDS; }

HD u32 cuckoo_loc(const u32 *tab, const unsigned char *item, u32 table_size)
{
    u32 w[4];
#pragma unroll
    for (int k = 0; k < 4; k++) w[k] = (u32)item[4 * k] | ((u32)item[4 * k + 1] << 8) | ((u32)item[4 * k + 2] << 16) | ((u32)item[4 * k + 3] << 24);
    return cuckoo_hash(tab, w[0], w[1], w[2], w[3]) % table_size;
}

HD u64 cuckoo_key(u64 max_rounds, u64 r, u32 i) { return ((max_rounds - 1 - r) << 32) | i; }
HD u32 cuckoo_key_item(u64 key) { return (u32)key; }

// the settle decision of one item: its own key, what its slot holds, and whether the winner's bytes equal its own
enum CuckooState : u32 { CUCKOO_ACTIVE = 0, CUCKOO_PLACED = 1, CUCKOO_DUPLICATE = 2 };
HD u32 cuckoo_settle(u64 own_key, u64 slot, bool winner_equal)
{
    if (slot == own_key) return CUCKOO_PLACED;
    return winner_equal ? CUCKOO_DUPLICATE : CUCKOO_ACTIVE;
}
HD bool cuckoo_items_equal(const unsigned char *a, const unsigned char *b)
{
    bool eq = true;
#pragma unroll
    for (int k = 0; k < 16; k++) eq = eq && a[k] == b[k];
    return eq;
}

// algebraize_item's bit split (k_algebraize, kernels_db.hip): felt j of the item (lo, hi) = its 128 bits, little-endian; j * bpf < 128
HD u64 cuckoo_item_felt(u64 lo, u64 hi, u32 j, u32 bpf, u32 item_bits)
{
    const u32 off = j * bpf;
    const u32 take = off >= item_bits ? 0 : (item_bits - off < bpf ? item_bits - off : bpf);
    const u64 v = off >= 64 ? hi >> (off - 64) : (off ? (lo >> off) | (hi << (64 - off)) : lo);
    return take ? v & (~(u64)0 >> (64 - take)) : 0;
}
// values[b][p] of the querier's table (sender_osn.cpp:433-460 and BatchEncoder's padding): slot b * items_per_bundle + k of the table
// fills positions k F .. k F + F - 1 of row b, zeros from bins_per_bundle = items_per_bundle * F to n.  -> the table slot, or CUCKOO_NONE
HD u32 query_value_slot(u32 b, u32 p, u32 items_per_bundle, u32 F, u32 *j)
{
    const u32 k = p / F;
    if (k >= items_per_bundle) return CUCKOO_NONE;
    *j = p - k * F;
    return b * items_per_bundle + k;
}

// ---- host only: the database side's grouping (apsu_he_items_bucket).  locs[count][H]; a stable counting sort by location:
// offsets[T + 1], order[offsets[l] .. offsets[l + 1]) = the items of location l in input order, an item whose functions collide on l
// once (the unordered_set of all_locations, receiver_db.cpp:57-79).  order holds count * H words; -> total = offsets[T].
// false: a location >= T.
inline bool cuckoo_bucket(const u32 *locs, size_t count, u32 H, u32 T, u64 *offsets, u32 *order, u64 *total)
{
    for (size_t l = 0; l <= T; l++) offsets[l] = 0;
    auto first_use = [&](const u32 *li, u32 h) { for (u32 g = 0; g < h; g++) if (li[g] == li[h]) return false; return true; };
    for (size_t i = 0; i < count; i++)
        for (u32 h = 0; h < H; h++) {
            if (locs[i * H + h] >= T) return false;
            if (first_use(locs + i * H, h)) offsets[(size_t)locs[i * H + h] + 1]++;
        }
    for (size_t l = 0; l < T; l++) offsets[l + 1] += offsets[l];
    // offsets[l] walks to the end of bucket l while it fills and is moved back afterwards
    for (size_t i = 0; i < count; i++)
        for (u32 h = 0; h < H; h++)
            if (first_use(locs + i * H, h)) order[offsets[locs[i * H + h]]++] = (u32)i;
    for (size_t l = T; l > 0; l--) offsets[l] = offsets[l - 1];
    offsets[0] = 0;
    *total = offsets[T];
    return true;
}

} // namespace apsu_he
