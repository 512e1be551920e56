// One kernel of the multiply-accumulate family at a time on caller-chosen words (Engine::debug_run_step from STEP_MAC_INFO on;
// include/apsu_he.h).  As the other engine_*_steps.cpp do for their families: a step copies host arrays up, calls THE launcher the
// engine calls -- launch_mac, launch_term_product, launch_pack_rows, launch_unpack_rows (launch_mac.h), launch_limb0_rows (launch_db.h)
// -- with this context's own DevLevel block dlevel(chain_idx), synchronises and copies back.  out[0] is copied up first everywhere, so
// a word the kernel does not write comes back as it went.  Bit-packed bytes travel as 64-bit words; every bit-packed buffer a kernel
// reads is uploaded with 16 readable (zero) bytes behind it, as the engine keeps them.  The row geometry is read back from the device
// block itself (mac_info, the packed operands' decoding), so what is checked is what the kernels read.  Whatever a launcher's
// contract does not admit is refused before anything is launched.  For the tests; nothing on the query path calls it.
#include "engine_impl.h"
#include "mac_plan.h"

#include <string>

namespace apsu_he {

namespace {

[[noreturn]] void refuse(const std::string &why) { throw std::invalid_argument("debug_run_step: " + why); }
void need(bool ok, const char *why) { if (!ok) refuse(why); }

void canonical(const u64 *x, size_t words, u64 m, const char *what)
{
    u64 bad = 0;
    for (size_t k = 0; k < words; k++) bad |= (u64)(x[k] >= m);
    if (bad) refuse(std::string(what) + " holds a word that is not a canonical residue of its limb");
}

// dense slots [slots][L][n]
void canonical_dense(const u64 *x, size_t slots, int L, size_t n, const DevLevel &lv, const char *what)
{
    for (size_t s = 0; s < slots; s++)
        for (int j = 0; j < L; j++) canonical(x + (s * L + j) * n, n, lv.q[j].q, what);
}

// bit-packed slots, `padded`: the slots and 16 bytes behind them (packed_coeff reads up to 8 bytes past a row's last coefficient)
void canonical_packed(const std::vector<u64> &padded, size_t slots, size_t slot_bytes, int L, size_t n, const DevLevel &lv, const char *what)
{
    const char *base = reinterpret_cast<const char *>(padded.data());
    u64 bad = 0;
    for (size_t s = 0; s < slots; s++)
        for (int j = 0; j < L; j++) {
            const u32 *row = reinterpret_cast<const u32 *>(base + s * slot_bytes + lv.mac_row_off[j]);
            for (size_t c = 0; c < n; c++) bad |= (u64)(packed_coeff(row, c, lv.mac_bits[j]) >= lv.q[j].q);
        }
    if (bad) refuse(std::string(what) + " holds a coefficient that is not a canonical residue of its limb");
}

} // namespace

void Engine::debug_run_mac_step(const StepArgs &a)
{
    const size_t n = hp_.n;
    need(a.step >= STEP_MAC_INFO && a.step <= STEP_LIMB0_ROWS, "unknown step");
    check_level(a.chain_idx);
    const int L = a.chain_idx + 1;
    const bool kara = a.flags & STEP_KARA, packed = a.flags & STEP_PACKED, limb_slow = a.flags & STEP_LIMB_SLOW;
    const size_t batch = a.batch > 0 ? (size_t)a.batch : 0, terms = a.terms > 0 ? (size_t)a.terms : 0, polys = a.polys > 0 ? (size_t)a.polys : 0;
    auto in_is = [&](int i, size_t words, const char *what) { if (!a.in[i] || a.in_words[i] != words) refuse(std::string(what) + ": wrong size"); };
    auto out_is = [&](int i, size_t words, const char *what) { if (!a.out[i] || a.out_words[i] != words) refuse(std::string(what) + ": wrong size"); };

    // the level block as the kernels read it
    sync();
    DevLevel lv;
    HIP_CHECK(hipMemcpy(&lv, dlevel(a.chain_idx), sizeof(DevLevel), hipMemcpyDeviceToHost));
    if (lv.L != L) throw std::logic_error("debug_run_step: the device's level block is not the level's");
    size_t packed_slot = 0;
    bool any_packed = false;
    for (int j = 0; j < L; j++) { packed_slot += n * lv.mac_bits[j] / 8; any_packed |= lv.mac_bits[j] != 64; }
    const size_t dense_slot = (size_t)L * n * sizeof(u64);

    if (a.step == STEP_MAC_INFO) {
        // out[0] = L, the bit-packed slot's bytes, then per limb: mac_shift, mac_chunk, mac_chunk_k, mac_bits, mac_row_off, mac_mask_hi, mac_kara_usable
        out_is(0, 2 + 7 * (size_t)L, "mac_info: out[0] [2 + 7 L]");
        u64 *o = a.out[0];
        *o++ = (u64)L; *o++ = packed_slot;
        for (int j = 0; j < L; j++) {
            *o++ = lv.mac_shift[j]; *o++ = lv.mac_chunk[j]; *o++ = lv.mac_chunk_k[j]; *o++ = lv.mac_bits[j]; *o++ = lv.mac_row_off[j];
            *o++ = lv.mac_mask_hi[j]; *o++ = mac_kara_usable(lv.q[j].q) ? 1 : 0;
        }
        return;
    }
    need(n % 64 == 0, "the multiply-accumulate steps take rings of a multiple of 64 coefficients (a bit-packed slot is whole 64-bit words)");
    if (packed) need(any_packed, "packed: every row of this context is 64 bits wide (mac_bits), there is no bit-packed form");
    const size_t slot = packed ? packed_slot : dense_slot, slot_words = slot / 8;      // bytes, 64-bit words of one plaintext slot

    // ---- everything a launcher's contract does not admit is refused here, in front of the arena: nothing below can refuse
    std::vector<MacJob> mj;
    std::vector<TermJob> tj;
    std::vector<u64> padded;                                         // the bit-packed operand with its 16 bytes behind (uploaded from here)
    auto pad_in = [&](int i) { padded.assign(a.in_words[i] + 2, 0); std::memcpy(padded.data(), a.in[i], a.in_words[i] * sizeof(u64)); };
    size_t P = 0, NL = 0, njobs = 0;
    switch (a.step) {
    case STEP_MAC: {
        // polys = streams per job (the arrays' extent), terms = terms per chain (the arrays' extent), e0 = limb0, n_ext = nl;
        // in[0] powers [batch][terms][2][P][n], in[1] plaintexts [batch][polys][terms] slots, in[2] null or the job table [batch][4] =
        // limb0, nl, ng, cnt -> out[0] [batch][polys][2][n_ext][n] in/out
        need(batch >= 1 && batch <= 64, "mac: batch out of range (1 .. 64)");
        need(polys >= 1 && polys <= (size_t)MAC_G, "mac: streams per job (polys) outside 1 .. 4");
        need(terms >= 1, "mac: a chain of no terms (terms 0)");
        need(terms <= 4096, "mac: terms out of range (1 .. 4096)");
        NL = a.n_ext > 0 ? (size_t)a.n_ext : 0;
        need(a.e0 >= 0 && NL >= 1 && (size_t)a.e0 + NL <= (size_t)L, "mac: limbs limb0 .. limb0 + nl - 1 (e0, n_ext) reach beyond the level");
        const size_t pw_job = batch * terms * 2 * n;
        need(a.in[0] && a.in_words[0] % pw_job == 0, "mac: in[0] powers [batch][terms][2][P][n]: wrong size");
        P = a.in_words[0] / pw_job;
        need(P >= (size_t)L, "mac: powers of fewer limbs per polynomial (P) than the level has");
        need(P <= (size_t)DMAXE, "mac: powers of more limbs per polynomial (P) than an extended polynomial has");
        in_is(1, batch * polys * terms * slot_words, "mac: in[1] plaintexts [batch][polys][terms] slots");
        out_is(0, batch * polys * 2 * NL * n, "mac: out[0] [batch][polys][2][n_ext][n]");
        if (a.in[2]) in_is(2, batch * 4, "mac: in[2] job table [batch][4]");
        if (kara) for (int j = 0; j < L; j++) need(mac_kara_usable(lv.q[j].q), "mac: the three-product form on a level with a prime that mac_kara_usable rejects");
        for (size_t r = 0; r < batch * terms * 2; r++)
            for (int j = 0; j < L; j++) canonical(a.in[0] + (r * P + j) * n, n, lv.q[j].q, "mac: in[0] (powers)");
        if (packed) { pad_in(1); canonical_packed(padded, batch * polys * terms, slot, L, n, lv, "mac: in[1] (bit-packed plaintexts)"); }
        else canonical_dense(a.in[1], batch * polys * terms, L, n, lv, "mac: in[1] (plaintexts)");
        for (size_t b = 0; b < batch; b++) {
            const u64 limb0 = a.in[2] ? a.in[2][b * 4] : (u64)a.e0, nl = a.in[2] ? a.in[2][b * 4 + 1] : NL;
            const u64 ng = a.in[2] ? a.in[2][b * 4 + 2] : polys, cnt = a.in[2] ? a.in[2][b * 4 + 3] : terms;
            need(limb0 <= (u64)L && nl >= 1 && nl <= NL && limb0 + nl <= (u64)L, "mac: a job's limbs (limb0, nl) reach beyond the level or beyond n_ext");
            need(ng >= 1 && ng <= polys, "mac: a job's streams (ng) outside 1 .. polys");
            need(cnt >= 1, "mac: a job with a chain of no terms (cnt 0)");
            need(cnt <= terms, "mac: a job's chain (cnt) is longer than terms");
            MacJob j{};
            j.cnt = (u32)cnt; j.ng = (u32)ng; j.limb0 = (u32)limb0; j.nl = (u32)nl; j.packed = packed ? 1 : 0;
            j.pt_stride = (u32)(packed ? slot : slot_words); j.pw_stride = (u32)(2 * P * n); j.pw_poly_stride = (u32)(P * n); j.out_poly_stride = (u32)(NL * n);
            mj.push_back(j);                                         // (the pointers: below, once the arrays have addresses)
        }
    } break;
    case STEP_TERM_PRODUCT: {
        // e0 = the limb; `batch` operand sets, each repeated `terms` times: job u < batch * terms reads set u % batch;
        // in[0] powers [batch][2][P][n], in[1] plaintexts [batch] slots -> out[0] [batch * terms + 1][2][n] in/out (the last [2][n]: a guard)
        need(batch >= 1 && batch <= 64, "term_product: batch out of range (1 .. 64)");
        need(terms >= 1 && batch * terms <= ((size_t)1 << 17), "term_product: jobs (batch * terms) outside 1 .. 2^17");
        need(a.e0 >= 0 && a.e0 < L, "term_product: the limb (e0) is beyond the level");
        need(a.in[0] && a.in_words[0] % (batch * 2 * n) == 0, "term_product: in[0] powers [batch][2][P][n]: wrong size");
        P = a.in_words[0] / (batch * 2 * n);
        need(P >= (size_t)L && P <= (size_t)DMAXE, "term_product: limbs per polynomial of the powers (P) outside L .. the extended base");
        njobs = batch * terms;
        in_is(1, batch * slot_words, "term_product: in[1] plaintexts [batch] slots");
        out_is(0, (njobs + 1) * 2 * n, "term_product: out[0] [batch * terms + 1][2][n]");
        for (size_t r = 0; r < batch * 2; r++) canonical(a.in[0] + (r * P + (size_t)a.e0) * n, n, lv.q[a.e0].q, "term_product: in[0] (powers)");
        if (packed) { pad_in(1); canonical_packed(padded, batch, slot, L, n, lv, "term_product: in[1] (bit-packed plaintexts)"); }
        else canonical_dense(a.in[1], batch, L, n, lv, "term_product: in[1] (plaintexts)");
    } break;
    case STEP_PACK_ROWS:
    case STEP_UNPACK_ROWS: {
        // batch = slots; PACK: in[0] dense [slots][L][n] -> out[0] the bit-packed slots and 16 bytes behind them, in/out;
        // UNPACK: in[0] the bit-packed slots -> out[0] dense [slots][L][n] in/out
        need(batch >= 1, "pack_rows / unpack_rows: no slots (batch)");
        pack_rows_grid_check(batch, L);                              // before the sizes: the refusal needs no arrays of that extent
        if (a.step == STEP_PACK_ROWS) {
            in_is(0, batch * (size_t)L * n, "pack_rows: in[0] dense [slots][L][n]");
            out_is(0, batch * packed_slot / 8 + 2, "pack_rows: out[0] [slots] bit-packed slots + 16 bytes");
            canonical_dense(a.in[0], batch, L, n, lv, "pack_rows: in[0]");
        } else {
            in_is(0, batch * packed_slot / 8, "unpack_rows: in[0] [slots] bit-packed slots");
            out_is(0, batch * (size_t)L * n, "unpack_rows: out[0] dense [slots][L][n]");
            pad_in(0);
        }
    } break;
    case STEP_LIMB0_ROWS: {
        // batch = count; in[0] [count] slots, dense [L][n] or (PACKED) bit-packed -> out[0] [count][n] in/out
        need(batch >= 1 && batch <= 65535, "limb0_rows: count (batch) outside 1 .. 65535");
        in_is(0, batch * slot_words, "limb0_rows: in[0] [count] slots");
        out_is(0, batch * n, "limb0_rows: out[0] [count][n]");
        if (packed) pad_in(0);
    } break;
    default: refuse("unknown step");
    }

    WITH_ARENA({
        auto up = [&](const u64 *src, size_t words) {
            u64 *d = ws(words);
            HIP_CHECK(hipMemcpyAsync(d, src, words * sizeof(u64), hipMemcpyHostToDevice, st_));
            return d;
        };
        auto up_slots = [&](int i) { return packed || a.step == STEP_UNPACK_ROWS ? up(padded.data(), padded.size()) : up(a.in[i], a.in_words[i]); };
        auto down = [&](const u64 *src) { HIP_CHECK(hipMemcpyAsync(a.out[0], src, a.out_words[0] * sizeof(u64), hipMemcpyDeviceToHost, st_)); };
        auto jobs = [&](const auto &v) {
            using T = typename std::decay_t<decltype(v)>::value_type;
            T *d = ws_as<T>(v.size());
            HIP_CHECK(hipMemcpyAsync(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st_));
            return static_cast<const T *>(d);
        };
        u64 *o = up(a.out[0], a.out_words[0]);

        switch (a.step) {
        case STEP_MAC: {
            const u64 *pw = up(a.in[0], a.in_words[0]);
            const char *pt = reinterpret_cast<const char *>(up_slots(1));
            for (size_t b = 0; b < batch; b++) {
                MacJob &j = mj[b];
                j.pw = pw + b * terms * 2 * P * n;
                // a stream the job does not have reads stream 0's plaintexts, as mac_plan sets it (k_mac reads no other); its output pointer
                // is its own slot of out[0] while the array has one (g < polys: a store the kernel should not make shows there), stream 0's beyond
                for (size_t g = 0; g < (size_t)MAC_G; g++) {
                    j.pt[g] = reinterpret_cast<const u64 *>(pt + ((b * polys + (g < j.ng ? g : 0)) * terms) * slot);
                    j.out[g] = o + (b * polys + (g < polys ? g : 0)) * 2 * NL * n;
                }
            }
            launch_mac(dlevel(a.chain_idx), L, jobs(mj), n, (int)batch, st_, kara, packed, MacGrid{ mac_grid(n, batch).gx, limb_slow ? 1 : 0 });
        } break;
        case STEP_TERM_PRODUCT: {
            const u64 *pw = up(a.in[0], a.in_words[0]);
            const char *pt = reinterpret_cast<const char *>(up_slots(1));
            tj.clear();                                              // a retry with a larger arena starts over
            for (size_t u = 0; u < njobs; u++) tj.push_back(TermJob{ reinterpret_cast<const u64 *>(pt + (u % batch) * slot), pw + (u % batch) * 2 * P * n, o + u * 2 * n });
            launch_term_product(dlevel(a.chain_idx), jobs(tj), njobs, n, a.e0, (u32)(P * n), (u32)n, packed, st_);
        } break;
        case STEP_PACK_ROWS:
            launch_pack_rows(dlevel(a.chain_idx), L, up(a.in[0], a.in_words[0]), o, packed_slot, n, batch, st_);
            break;
        case STEP_UNPACK_ROWS:
            launch_unpack_rows(dlevel(a.chain_idx), L, up_slots(0), packed_slot, o, n, batch, st_);
            break;
        default:                                                     // STEP_LIMB0_ROWS
            launch_limb0_rows(dlevel(a.chain_idx), L, up_slots(0), slot, packed, o, n, batch, st_);
            break;
        }
        down(o);
        sync();
    });
}

} // namespace apsu_he
