// The database side's grouping by location on the device, a translation unit of its own: the surviving entries as keys loc << 32 | i,
// a stable least-significant-digit radix sort of them on the bits of loc, offsets and order from the sorted keys, and the gather of
// the entries.  Rules and the design: bucket_plan.h, which the CPU tier steps as well; contracts: launch_bucket.h.
// Nothing here takes a rank from an atomic (there is no atomic at all) and no workgroup waits for another: what needs the whole of
// an earlier step's result is a launch of its own behind it on the stream.
#include "launch_bucket.h"
#include "kernel_launch.h"

#include <stdexcept>
#include <string>

namespace apsu_he {

// ---- the keys.  Tiles of `tile` ITEMS; a lane takes one item at a time, the tile's 256 lanes walk it 256 items a step.
// the locations of item i into registers (every index is a constant once unrolled)
__device__ __forceinline__ void bucket_load_locs(const u32 *__restrict__ locs, size_t i, u32 H, u32 li[BUCKET_MAX_FUNCS])
{
#pragma unroll
    for (u32 h = 0; h < BUCKET_MAX_FUNCS; h++) li[h] = h < H ? locs[i * H + h] : 0;
}
__device__ __forceinline__ u32 bucket_count_regs(const u32 li[BUCKET_MAX_FUNCS], u32 H)
{
    u32 c = 0;
#pragma unroll
    for (u32 h = 0; h < BUCKET_MAX_FUNCS; h++) c += h < H && bucket_first_use(li, h) ? 1 : 0;
    return c;
}

// inclusive sums over the lanes of a wave
template <class V> __device__ __forceinline__ V wave_inclusive(V v, u32 lane)
{
#pragma unroll
    for (u32 d = 1; d < BUCKET_WAVE; d <<= 1) {
        const V up = __shfl_up(v, d);
        if (lane >= d) v += up;
    }
    return v;
}

// tile_cnt[t] = the surviving entries of the items of tile t
__global__ __launch_bounds__(BUCKET_T) void k_bucket_count(const u32 *__restrict__ locs, size_t count, u32 H, u32 tile, u32 *__restrict__ tile_cnt)
{
    __shared__ u32 wtot[BUCKET_WAVES];
    const u32 tid = threadIdx.x, lane = tid & (BUCKET_WAVE - 1), w = tid / BUCKET_WAVE;
    const size_t first = (size_t)blockIdx.x * tile, end = first + tile < count ? first + tile : count;
    u32 c = 0;
    for (size_t i = first + tid; i < end; i += BUCKET_T) {
        u32 li[BUCKET_MAX_FUNCS];
        bucket_load_locs(locs, i, H, li);
        c += bucket_count_regs(li, H);
    }
    c = wave_inclusive(c, lane);
    if (lane == BUCKET_WAVE - 1) wtot[w] = c;
    __syncthreads();
    if (tid == 0) {
        u32 all = 0;
        for (u32 ww = 0; ww < BUCKET_WAVES; ww++) all += wtot[ww];
        tile_cnt[blockIdx.x] = all;
    }
}

// keys[tile_base[t] ..] = the keys of tile t's items in (i, h) order
__global__ __launch_bounds__(BUCKET_T) void k_bucket_keys(const u32 *__restrict__ locs, size_t count, u32 H, u32 tile, const u64 *__restrict__ tile_base,
                                                          u64 *__restrict__ keys)
{
    __shared__ u32 wtot[2][BUCKET_WAVES];                             // step s votes in wtot[s & 1]: one barrier a step
    const u32 tid = threadIdx.x, lane = tid & (BUCKET_WAVE - 1), w = tid / BUCKET_WAVE;
    const size_t first = (size_t)blockIdx.x * tile, end = first + tile < count ? first + tile : count;
    u64 base = tile_base[blockIdx.x];
    u32 step = 0;
    for (size_t i0 = first; i0 < end; i0 += BUCKET_T, step++) {      // workgroup-uniform
        const size_t i = i0 + tid;
        u32 li[BUCKET_MAX_FUNCS];
        u32 c = 0;
        if (i < end) { bucket_load_locs(locs, i, H, li); c = bucket_count_regs(li, H); }
        const u32 inc = wave_inclusive(c, lane);
        if (lane == BUCKET_WAVE - 1) wtot[step & 1][w] = inc;
        __syncthreads();
        u32 before = 0, all = 0;
#pragma unroll
        for (u32 ww = 0; ww < BUCKET_WAVES; ww++) { const u32 v = wtot[step & 1][ww]; before += ww < w ? v : 0; all += v; }
        if (i < end) {
            u64 pos = base + before + inc - c;
#pragma unroll
            for (u32 h = 0; h < BUCKET_MAX_FUNCS; h++)
                if (h < H && bucket_first_use(li, h)) keys[pos++] = bucket_key(li[h], (u32)i);
        }
        base += all;
    }
}

// ---- out[k] = the sum of in[0 .. k - 1] for k < n, *sum = the sum of all (sum may be null).  One workgroup walks the array.
__global__ __launch_bounds__(BUCKET_SCAN_T) void k_bucket_scan(const u32 *__restrict__ in, u64 n, u64 *__restrict__ out, u64 *__restrict__ sum)
{
    constexpr u32 WAVES = BUCKET_SCAN_T / BUCKET_WAVE, PER = BUCKET_SCAN_PER_LANE;
    __shared__ u64 wtot[2][WAVES];
    const u32 tid = threadIdx.x, lane = tid & (BUCKET_WAVE - 1), w = tid / BUCKET_WAVE;
    u64 carry = 0;
    u32 step = 0;
    for (u64 c0 = 0; c0 < n; c0 += (u64)BUCKET_SCAN_T * PER, step++) {
        const u64 first = c0 + (u64)tid * PER;
        u32 v[PER];
        u64 s = 0;
#pragma unroll
        for (u32 j = 0; j < PER; j++) { v[j] = first + j < n ? in[first + j] : 0; s += v[j]; }
        const u64 inc = wave_inclusive((unsigned long long)s, lane);
        if (lane == BUCKET_WAVE - 1) wtot[step & 1][w] = inc;
        __syncthreads();
        u64 before = 0, all = 0;
#pragma unroll
        for (u32 ww = 0; ww < WAVES; ww++) { const u64 x = wtot[step & 1][ww]; before += ww < w ? x : 0; all += x; }
        u64 run = carry + before + inc - s;
#pragma unroll
        for (u32 j = 0; j < PER; j++) {
            if (first + j < n) out[first + j] = run;
            run += v[j];
        }
        carry += all;
    }
    if (tid == 0 && sum) *sum = carry;
}

// ---- a pass.  One round of a wave over 64 keys of its run: -> this lane's digit, its rank among the wave's lanes with that digit
// and how many they are (bucket_match over the digit's bits).  Every lane of the wave arrives (the loop around it is wave-uniform).
__device__ __forceinline__ u32 bucket_round(u64 key, bool valid, u32 shift, u32 width, u32 lane, u32 *rank, u32 *peers)
{
    const u32 d = bucket_digit(key, shift, width);
    u64 mask = __ballot(valid);
    for (u32 bit = 0; bit < width; bit++) {                          // wave-uniform
        const bool set = (d >> bit) & 1;
        mask = bucket_match(mask, __ballot(set), set);
    }
    *rank = bucket_rank(mask, lane);
    *peers = bucket_peers(mask);
    return d;
}

// hist[d][t] = the keys of tile t with digit d, wave_cnt[t][w][d] = those of them in wave w's run.  Every tile of the grid writes its
// counters, one beyond *total zeros.  A wave counts in a row of its own: the lowest lane of each digit adds the round's count.
__global__ __launch_bounds__(BUCKET_T) void k_bucket_hist(const u64 *__restrict__ keys, const u64 *__restrict__ total, u32 tile, u32 shift, u32 width,
                                                          u32 *__restrict__ hist, u32 *__restrict__ wave_cnt)
{
    __shared__ u32 cnt[BUCKET_WAVES][1 << BUCKET_DIGIT_BITS];
    const u32 tid = threadIdx.x, lane = tid & (BUCKET_WAVE - 1), w = tid / BUCKET_WAVE, D = 1u << width;
    const u64 t = blockIdx.x, tiles = gridDim.x;
    volatile u32 *mine = cnt[w];
    for (u32 d = lane; d < D; d += BUCKET_WAVE) mine[d] = 0;
    const u32 len = bucket_tile_len(*total, tile, t);
    u32 b, e;
    bucket_wave_run(tile, len, w, &b, &e);
    const u64 *src = keys + t * tile;
    for (u32 r = b; r < e; r += BUCKET_WAVE) {                       // wave-uniform
        const bool valid = r + lane < e;
        const u64 key = valid ? src[r + lane] : 0;
        u32 rank, peers;
        const u32 d = bucket_round(key, valid, shift, width, lane, &rank, &peers);
        if (valid && rank == 0) mine[d] = mine[d] + peers;
    }
    __syncthreads();
    for (u32 d = tid; d < D; d += BUCKET_T) {
        u32 all = 0;
#pragma unroll
        for (u32 ww = 0; ww < BUCKET_WAVES; ww++) {
            const u32 c = cnt[ww][d];
            wave_cnt[(t * BUCKET_WAVES + ww) * D + d] = c;
            all += c;
        }
        hist[(u64)d * tiles + t] = all;
    }
}

// out[scanned[d][t] + (the keys of digit d in the tile's earlier waves, and in this wave's earlier rounds and lower lanes)] = key: stable.
// base[w][d] is wave w's next free place of digit d; the highest lane of each digit moves it on behind the round's reads.
__global__ __launch_bounds__(BUCKET_T) void k_bucket_scatter(const u64 *__restrict__ keys, const u64 *__restrict__ total, u32 tile, u32 shift, u32 width,
                                                             const u64 *__restrict__ scanned, const u32 *__restrict__ wave_cnt, u64 *__restrict__ out)
{
    __shared__ u64 base[BUCKET_WAVES][1 << BUCKET_DIGIT_BITS];
    const u32 tid = threadIdx.x, lane = tid & (BUCKET_WAVE - 1), w = tid / BUCKET_WAVE, D = 1u << width;
    const u64 t = blockIdx.x, tiles = gridDim.x;
    const u32 len = bucket_tile_len(*total, tile, t);
    if (!len) return;                                                // workgroup-uniform
    for (u32 d = tid; d < D; d += BUCKET_T) {
        u64 run = scanned[(u64)d * tiles + t];
#pragma unroll
        for (u32 ww = 0; ww < BUCKET_WAVES; ww++) { base[ww][d] = run; run += wave_cnt[(t * BUCKET_WAVES + ww) * D + d]; }
    }
    __syncthreads();
    volatile u64 *mine = base[w];
    u32 b, e;
    bucket_wave_run(tile, len, w, &b, &e);
    const u64 *src = keys + t * tile;
    for (u32 r = b; r < e; r += BUCKET_WAVE) {                       // wave-uniform
        const bool valid = r + lane < e;
        const u64 key = valid ? src[r + lane] : 0;
        u32 rank, peers;
        const u32 d = bucket_round(key, valid, shift, width, lane, &rank, &peers);
        u64 at = 0;
        if (valid) at = mine[d];
        if (valid) out[at + rank] = key;
        if (valid && rank + 1 == peers) mine[d] = at + peers;
    }
}

// offsets[l] = the sorted keys below l << 32, l <= T
__global__ __launch_bounds__(BUCKET_T) void k_bucket_offsets(const u64 *__restrict__ keys, const u64 *__restrict__ total, u32 T, u64 *__restrict__ offsets)
{
    const u64 n = *total;
    for (u64 l = (u64)blockIdx.x * BUCKET_T + threadIdx.x; l <= T; l += (u64)gridDim.x * BUCKET_T) offsets[l] = bucket_lower_bound(keys, n, l << 32);
}

__global__ __launch_bounds__(BUCKET_T) void k_bucket_order(const u64 *__restrict__ keys, const u64 *__restrict__ total, u32 *__restrict__ order)
{
    const u64 n = *total;
    for (u64 k = (u64)blockIdx.x * BUCKET_T + threadIdx.x; k < n; k += (u64)gridDim.x * BUCKET_T) order[k] = bucket_key_item(keys[k]);
}

__global__ __launch_bounds__(BUCKET_T) void k_entries_gather(const uint4 *__restrict__ items, const u32 *__restrict__ order, const u64 *__restrict__ total,
                                                             uint4 *__restrict__ entries)
{
    const u64 n = *total;
    for (u64 k = (u64)blockIdx.x * BUCKET_T + threadIdx.x; k < n; k += (u64)gridDim.x * BUCKET_T) entries[k] = items[order[k]];
}

// a grid of BUCKET_T lanes for `n` elements under a stride loop: one lane each up to 2^20 workgroups
static dim3 stride_grid(u64 n) { return dim3((unsigned)std::min<u64>((n + BUCKET_T - 1) / BUCKET_T, (u64)1 << 20)); }

// ---- one launcher per kernel (contracts: launch_bucket.h): launch_bucket_sort below and the steps of engine_bucket_steps.cpp run these
static void key_contract(size_t count, u32 H, u32 tile, const char *who)
{
    if (!count || count >= 0xFFFFFFFFull || !H || H > BUCKET_MAX_FUNCS || !bucket_tile_ok(tile)) throw std::logic_error(std::string(who) + ": outside its contract");
}
static void pass_contract(u64 tiles, u32 tile, u32 shift, u32 width, const char *who)
{
    if (!tiles || tiles > 0x7FFFFFFFull || !bucket_tile_ok(tile) || !width || width > BUCKET_DIGIT_BITS || shift < 32 || shift + width > 64)
        throw std::logic_error(std::string(who) + ": outside its contract");
}

void launch_bucket_count(const u32 *locs, size_t count, u32 H, u32 tile, u32 *tile_cnt, hipStream_t st)
{
    key_contract(count, H, tile, "launch_bucket_count");
    hipLaunchKernelGGL(k_bucket_count, dim3((unsigned)bucket_tiles(count, tile)), dim3(BUCKET_T), 0, st, locs, count, H, tile, tile_cnt);
    KERNEL_CHECK();
}

void launch_bucket_keys(const u32 *locs, size_t count, u32 H, u32 tile, const u64 *tile_base, u64 *keys, hipStream_t st)
{
    key_contract(count, H, tile, "launch_bucket_keys");
    hipLaunchKernelGGL(k_bucket_keys, dim3((unsigned)bucket_tiles(count, tile)), dim3(BUCKET_T), 0, st, locs, count, H, tile, tile_base, keys);
    KERNEL_CHECK();
}

void launch_bucket_scan(const u32 *in, u64 n, u64 *out, u64 *sum, hipStream_t st)
{
    hipLaunchKernelGGL(k_bucket_scan, dim3(1), dim3(BUCKET_SCAN_T), 0, st, in, n, out, sum);
    KERNEL_CHECK();
}

void launch_bucket_hist(const u64 *keys, const u64 *total, u64 tiles, u32 tile, u32 shift, u32 width, u32 *hist, u32 *wave_cnt, hipStream_t st)
{
    pass_contract(tiles, tile, shift, width, "launch_bucket_hist");
    hipLaunchKernelGGL(k_bucket_hist, dim3((unsigned)tiles), dim3(BUCKET_T), 0, st, keys, total, tile, shift, width, hist, wave_cnt);
    KERNEL_CHECK();
}

void launch_bucket_scatter(const u64 *keys, const u64 *total, u64 tiles, u32 tile, u32 shift, u32 width, const u64 *scanned, const u32 *wave_cnt, u64 *out,
                           hipStream_t st)
{
    pass_contract(tiles, tile, shift, width, "launch_bucket_scatter");
    hipLaunchKernelGGL(k_bucket_scatter, dim3((unsigned)tiles), dim3(BUCKET_T), 0, st, keys, total, tile, shift, width, scanned, wave_cnt, out);
    KERNEL_CHECK();
}

void launch_bucket_offsets(const u64 *keys, const u64 *total, u32 T, u64 *offsets, hipStream_t st)
{
    if (!T) throw std::logic_error("launch_bucket_offsets: outside its contract");
    hipLaunchKernelGGL(k_bucket_offsets, stride_grid((u64)T + 1), dim3(BUCKET_T), 0, st, keys, total, T, offsets);
    KERNEL_CHECK();
}

void launch_bucket_order(const u64 *keys, const u64 *total, u64 room, u32 *order, hipStream_t st)
{
    if (!room) return;
    hipLaunchKernelGGL(k_bucket_order, stride_grid(room), dim3(BUCKET_T), 0, st, keys, total, order);
    KERNEL_CHECK();
}

const u64 *launch_bucket_sort(const u32 *locs, size_t count, u32 H, u32 T, u32 tile, const BucketWork &w, u64 *offsets, u32 *order, hipStream_t st)
{
    if (!count || count >= 0xFFFFFFFFull || !H || H > BUCKET_MAX_FUNCS || !T || !bucket_tile_ok(tile)) throw std::logic_error("launch_bucket_sort: outside its contract");
    const BucketSizes s = bucket_sizes(count, H, T, tile);
    const BucketDigits plan = bucket_digit_plan(T);
    launch_bucket_count(locs, count, H, tile, w.tile_cnt, st);
    launch_bucket_scan(w.tile_cnt, s.key_tiles, w.tile_base, w.total, st);
    launch_bucket_keys(locs, count, H, tile, w.tile_base, w.keys[0], st);
    u32 at = 0;
    for (u32 p = 0; p < plan.passes; p++, at ^= 1) {
        launch_bucket_hist(w.keys[at], w.total, s.tiles, tile, plan.shift[p], plan.width[p], w.hist, w.wave_cnt, st);
        launch_bucket_scan(w.hist, (u64)s.tiles << plan.width[p], w.scanned, nullptr, st);
        launch_bucket_scatter(w.keys[at], w.total, s.tiles, tile, plan.shift[p], plan.width[p], w.scanned, w.wave_cnt, w.keys[at ^ 1], st);
    }
    launch_bucket_offsets(w.keys[at], w.total, T, offsets, st);
    launch_bucket_order(w.keys[at], w.total, s.entries, order, st);
    return w.keys[at];
}

void launch_entries_gather(const unsigned char *items, const u32 *order, const u64 *total, u64 room, unsigned char *entries, hipStream_t st)
{
    if (!room) return;
    if (((uintptr_t)items & 15) || ((uintptr_t)entries & 15)) throw std::logic_error("launch_entries_gather: outside its contract");
    hipLaunchKernelGGL(k_entries_gather, stride_grid(room), dim3(BUCKET_T), 0, st, reinterpret_cast<const uint4 *>(items), order, total,
                       reinterpret_cast<uint4 *>(entries));
    KERNEL_CHECK();
}

} // namespace apsu_he
