// Stand-alone timing of the engine's k_mac on a synthetic DB, to bisect its HBM efficiency (see readbw.hip for the ceilings).
#include "../../apsu_amd/csrc/kernels_mac.hip"
#ifndef MACBENCH_PLAIN      // -DMACBENCH_PLAIN: k_mac only (the ring / persistent variants are written for four streams per job)
#include "mac_ring.hip"
#include "mac_persist.hip"
#endif
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>
#include <algorithm>
namespace apsu_he { void throw_hip(hipError_t e, const char* f, int l) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e), f, l); abort(); } }
using namespace apsu_he;
// k_mac as the library launches it for these jobs (the grid of mac_plan.h)
static void bench_mac(const DevLevel *lv, int nl, const MacJob *jobs, size_t n, int njobs, hipStream_t st, bool kara = false, bool packed = false) { launch_mac(lv, nl, jobs, n, njobs, st, kara, packed, mac_grid(n, (size_t)njobs)); }
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)
__global__ void k_fillrand(u64* p, size_t words, u64 mask) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) {
        u64 z = i * 0x9e3779b97f4a7c15ULL + 0x1234; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL; z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL; p[i] = (z ^ (z >> 31)) & mask; }
}

// Round 6, PLACEMENT mode with PROBE=1: what does ADDRESS TRANSLATION cost on this copy of the database?  65 536 lanes each read one 8-byte word
// from a different page per iteration (page = `stride` bytes; the next page a large odd step further), the addresses independent of the data:
// nothing is reused, every access is a new line and, at 4 KiB ... 2 MiB strides, a new page -- the time per iteration is the translation
// path's (UTCL1 miss -> UTCL2 -> page walk), which depends on how large the fragments are the driver mapped this copy with.
__global__ __launch_bounds__(256) void k_tlb_probe(const u64 *__restrict__ base, size_t npages, size_t stride_words, int iters, u64 *__restrict__ sink)
{
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    size_t p = (gid * 7919) % npages;
    u64 acc = 0;
    for (int i = 0; i < iters; i++) {
        acc += __builtin_nontemporal_load(base + p * stride_words + (gid & 7));
        p += 104729; if (p >= npages) p -= npages; if (p >= npages) p %= npages;
    }
    if (acc == 0x123456789abcdefULL) sink[0] = acc;
}

// ---- bisect kernels: same loads as k_mac<2,2>, different bodies
template <int MODE>
__global__ __launch_bounds__(256) void k_morph(const MacJob *__restrict__ jobs, size_t n, u64 *sink)
{
    const size_t k = ((size_t)blockIdx.x * 256 + threadIdx.x) * 2;
    const MacJob *__restrict__ jp = jobs + blockIdx.z / 2;
    const int g0 = (blockIdx.z % 2) * 2;
    const int j = blockIdx.y;
    const u64 *p0 = jp->pw + (size_t)j * n + k, *p1 = p0 + jp->pw_poly_stride;
    const u64 *a0 = jp->pt[g0] + (size_t)j * n + k, *a1 = jp->pt[g0 + 1] + (size_t)j * n + k;
    const u32 cnt = jp->cnt, pts = jp->pt_stride, pws = jp->pw_stride;
    u64 acc = 0;
    if (MODE == 0) {            // simple loop, compiler-scheduled
        for (u32 i = 0; i < cnt; i++) {
            const u64x2 c0 = ldg16(p0 + (size_t)i * pws), c1 = ldg16(p1 + (size_t)i * pws);
            const u64x2 x = ldg16_nt(a0 + (size_t)i * pts), y = ldg16_nt(a1 + (size_t)i * pts);
            acc += (x[0] * c0[0]) ^ (x[1] * c1[1]) ^ (y[0] * c0[1]) ^ (y[1] * c1[0]);
        }
    } else if (MODE == 1) {     // unroll 4
#pragma unroll 4
        for (u32 i = 0; i < cnt; i++) {
            const u64x2 c0 = ldg16(p0 + (size_t)i * pws), c1 = ldg16(p1 + (size_t)i * pws);
            const u64x2 x = ldg16_nt(a0 + (size_t)i * pts), y = ldg16_nt(a1 + (size_t)i * pts);
            acc += (x[0] * c0[0]) ^ (x[1] * c1[1]) ^ (y[0] * c0[1]) ^ (y[1] * c1[0]);
        }
    } else if (MODE == 2) {     // no power loads at all
#pragma unroll 4
        for (u32 i = 0; i < cnt; i++) {
            const u64x2 x = ldg16_nt(a0 + (size_t)i * pts), y = ldg16_nt(a1 + (size_t)i * pts);
            acc += (x[0] * 3) ^ (x[1] * 5) ^ (y[0] * 7) ^ (y[1] * 11);
        }
    } else if (MODE == 3) {     // 4 streams per block (G = 4): half the power loads per DB byte
        const u64 *a2 = jp->pt[(g0 + 2) & 3] + (size_t)j * n + k, *a3 = jp->pt[(g0 + 3) & 3] + (size_t)j * n + k;
        if (g0) return;
#pragma unroll 2
        for (u32 i = 0; i < cnt; i++) {
            const u64x2 c0 = ldg16(p0 + (size_t)i * pws), c1 = ldg16(p1 + (size_t)i * pws);
            const u64x2 x = ldg16_nt(a0 + (size_t)i * pts), y = ldg16_nt(a1 + (size_t)i * pts);
            const u64x2 z = ldg16_nt(a2 + (size_t)i * pts), w = ldg16_nt(a3 + (size_t)i * pts);
            acc += (x[0] * c0[0]) ^ (x[1] * c1[1]) ^ (y[0] * c0[1]) ^ (y[1] * c1[0]) ^ (z[0] * c0[0]) ^ (z[1] * c1[1]) ^ (w[0] * c0[1]) ^ (w[1] * c1[0]);
        }
    }
    if (acc == 0x1234567) sink[0] = acc;
}
int main(int argc, char** argv) {
    const size_t n = 8192, L = 3, ptw = L * n;
    const int terms = getenv("TERMS") ? atoi(getenv("TERMS")) : 44, streams = 784 - 784 % MAC_G, nb = argc > 1 ? atoi(argv[1]) : 4; const size_t pad = argc > 2 ? atoi(argv[2]) : 0, ppad = argc > 3 ? atoi(argv[3]) : 0;   // pad: words added to the power stride; ppad: to the poly stride       // nb: bundle indices interleaved in the powers layout
    const size_t skew = getenv("SKEW") ? atoi(getenv("SKEW")) : 0;   // extra words between consecutive streams (breaks the 8.25 MB stride)
    const size_t words = (size_t)streams * terms * ptw;
    u64 *db, *pw, *out; DevLevel* lv; MacJob* dj;
    CHECK(hipMalloc(&db, (words + (size_t)streams * skew) * 8)); const size_t pstride = nb * 2 * L * n + pad + 2 * ppad; CHECK(hipMalloc(&pw, (size_t)terms * pstride * 8)); CHECK(hipMalloc(&out, (size_t)streams * 2 * L * n * 8));
    k_fillrand<<<4096, 256>>>(db, words + (size_t)streams * skew, ((u64)1 << 55) - 1); k_fillrand<<<1024, 256>>>(pw, (size_t)terms * pstride, ((u64)1 << 55) - 1);
    DevLevel h; memset(&h, 0, sizeof(h)); h.L = 3;
    u64 q[3] = { 0xfffffffff70001ULL, 0xfffffffff78001ULL, 0xfffffffffb4001ULL };
    for (int j = 0; j < 3; j++) { unsigned __int128 all = ~(unsigned __int128)0; unsigned __int128 r = all / q[j]; h.q[j] = Mod{ q[j], (u64)r, (u64)(r >> 64) }; h.mac_shift[j] = 28; h.mac_chunk[j] = 127; h.mac_chunk_k[j] = 63; }
    CHECK(hipMalloc(&lv, sizeof(h))); CHECK(hipMemcpy(lv, &h, sizeof(h), hipMemcpyHostToDevice));
    std::vector<MacJob> jobs;
    for (int s = 0; s < streams; s += MAC_G) {
        MacJob j{}; j.pw = pw; j.cnt = terms; j.ng = MAC_G; j.pt_stride = ptw; j.pw_stride = pstride; j.pw_poly_stride = L * n + ppad; j.nl = 3; j.out_poly_stride = L * n; j.limb0 = 0;
        for (int g = 0; g < MAC_G; g++) { j.pt[g] = db + (size_t)(s + g) * (terms * ptw + skew); j.out[g] = out + (size_t)(s + g) * 2 * L * n; }
        jobs.push_back(j);
    }
    CHECK(hipMalloc(&dj, jobs.size() * sizeof(MacJob))); CHECK(hipMemcpy(dj, jobs.data(), jobs.size() * sizeof(MacJob), hipMemcpyHostToDevice));
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    {
        std::vector<float> t;
        for (int rep = 0; rep < 16; rep++) {
            CHECK(hipEventRecord(e0)); bench_mac(lv, 3, dj, n, (int)jobs.size(), 0); CHECK(hipEventRecord(e1)); CHECK(hipDeviceSynchronize());
            float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
            if (rep >= 2) t.push_back(ms);
        }
        std::sort(t.begin(), t.end());
        printf("k_mac<%d,%d> ring=%d nb=%d pad=%zu: min %.3f ms (%.0f GB/s)  median %.3f ms (%.0f GB/s)  max %.3f\n", MAC_G, MAC_C, 2, nb, pad,
               t[0], words * 8 / (t[0] * 1e-3) / 1e9, t[t.size() / 2], words * 8 / (t[t.size() / 2] * 1e-3) / 1e9, t.back());
    }
    // (the grid-order comparison that lived here -- ORDER=1: orders 0 / 1 / 2 with real powers and with one term's powers -- is recorded in
    //  profiles/r04_mac_grid_order.txt; the library keeps order 1 and the plan (mac_plan.h) holds it)
    if (getenv("PLACEMENT")) {
        // Does the scan's speed depend on WHERE the database lies?  (Identical binaries run one after the other alternate between 1.12 and
        // 1.26 ms, profiles/r05_mac_ring3.txt.)  Several copies of the same database in ONE process, the same kernel on each in turn;
        // SKEW_LIST: the same with the streams of one copy moved apart by extra words (relative alignment of the concurrently read rows).
        const int copies = atoi(getenv("PLACEMENT"));
        std::vector<u64 *> dbs{ db };
        for (int c = 1; c < copies; c++) { u64 *d2; CHECK(hipMalloc(&d2, (words + (size_t)streams * 8192) * 8)); k_fillrand<<<4096, 256>>>(d2, words + (size_t)streams * 8192, ((u64)1 << 55) - 1); dbs.push_back(d2); }
        std::vector<size_t> skews{ 0 };
        if (getenv("SKEW_LIST")) { skews.clear(); char *t = strdup(getenv("SKEW_LIST")); for (char *q2 = strtok(t, ","); q2; q2 = strtok(nullptr, ",")) skews.push_back((size_t)atoll(q2)); }
        for (int pass = 0; pass < 3; pass++)
            for (size_t c = 0; c < dbs.size(); c++)
                for (size_t sk : skews) {
                    if (c == 0 && sk > skew) continue;              // the first copy was allocated without room for a skew
                    std::vector<MacJob> jc = jobs;
                    for (size_t x = 0; x < jc.size(); x++) for (int g = 0; g < MAC_G; g++) jc[x].pt[g] = dbs[c] + (x * MAC_G + g) * (terms * ptw + sk);
                    MacJob *djc; CHECK(hipMalloc(&djc, jc.size() * sizeof(MacJob))); CHECK(hipMemcpy(djc, jc.data(), jc.size() * sizeof(MacJob), hipMemcpyHostToDevice));
                    std::vector<float> t;
                    for (int rep = 0; rep < 8; rep++) {
                        CHECK(hipEventRecord(e0)); bench_mac(lv, 3, djc, n, (int)jc.size(), 0); CHECK(hipEventRecord(e1)); CHECK(hipDeviceSynchronize());
                        float ms; CHECK(hipEventElapsedTime(&ms, e0, e1)); if (rep >= 2) t.push_back(ms);
                    }
                    std::sort(t.begin(), t.end());
                    printf("pass %d  copy %zu at %p  skew %5zu words: median %.3f ms (%.0f GB/s)\n", pass, c, (void *)dbs[c], sk, t[t.size() / 2], words * 8 / (t[t.size() / 2] * 1e-3) / 1e9);
                    CHECK(hipFree(djc));
                    if (getenv("PROBE") && pass == 2 && sk == 0) {
                        for (size_t stride : { (size_t)4096, (size_t)65536, (size_t)(2u << 20) }) {
                            const size_t npages = words * 8 / stride;
                            std::vector<float> tp;
                            for (int rep = 0; rep < 7; rep++) {
                                CHECK(hipEventRecord(e0)); k_tlb_probe<<<256, 256>>>(dbs[c], npages, stride / 8, 64, out); CHECK(hipEventRecord(e1)); CHECK(hipDeviceSynchronize());
                                float ms; CHECK(hipEventElapsedTime(&ms, e0, e1)); if (rep >= 2) tp.push_back(ms);
                            }
                            std::sort(tp.begin(), tp.end());
                            printf("        probe copy %zu: one word per %7zu-byte page, 65536 lanes x 64 pages: median %.1f us (%.1f ns per wave-access)\n", c, stride, tp[tp.size() / 2] * 1e3,
                                   tp[tp.size() / 2] * 1e6 / 64.0);
                        }
                    }
                }
    }
#ifndef MACBENCH_PLAIN
    if (getenv("PERSIST")) {
        // long-lived workgroups (k_mac_p) against one workgroup per unit (k_mac): separate output, bit-compared; A B A B timing
        u64 *out2; CHECK(hipMalloc(&out2, (size_t)streams * 2 * L * n * 8));
        std::vector<MacJob> jobs2 = jobs;
        for (size_t x = 0; x < jobs2.size(); x++) for (int g = 0; g < MAC_G; g++) jobs2[x].out[g] = out2 + (jobs[x].out[g] - out);
        MacJob *dj2; CHECK(hipMalloc(&dj2, jobs2.size() * sizeof(MacJob))); CHECK(hipMemcpy(dj2, jobs2.data(), jobs2.size() * sizeof(MacJob), hipMemcpyHostToDevice));
        const bool kara = getenv("KARA2") != nullptr;
        for (int r : { 0, 16, 24, 32, 48, 64, 96 }) {
            std::vector<float> ta, tb;
            for (int rep = 0; rep < 14; rep++) {
                float ms;
                CHECK(hipEventRecord(e0)); bench_mac(lv, 3, dj, n, (int)jobs.size(), 0, kara); CHECK(hipEventRecord(e1)); CHECK(hipDeviceSynchronize());
                CHECK(hipEventElapsedTime(&ms, e0, e1)); if (rep >= 2) ta.push_back(ms);
                CHECK(hipEventRecord(e0)); launch_mac_persist(lv, dj2, n, (int)jobs2.size(), 0, kara, r); CHECK(hipEventRecord(e1)); CHECK(hipDeviceSynchronize());
                CHECK(hipEventElapsedTime(&ms, e0, e1)); if (rep >= 2) tb.push_back(ms);
            }
            std::sort(ta.begin(), ta.end()); std::sort(tb.begin(), tb.end());
            const size_t ow = (size_t)streams * 2 * L * n;
            std::vector<u64> h1(ow), h2(ow);
            CHECK(hipMemcpy(h1.data(), out, ow * 8, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(h2.data(), out2, ow * 8, hipMemcpyDeviceToHost));
            size_t bad = 0; for (size_t x = 0; x < ow; x++) bad += h1[x] != h2[x];
            printf("persistent R=%2d: median %.3f ms (%.0f GB/s)   per unit: %.3f ms (%.0f GB/s)   %+.1f %%   %zu words differ\n", r, tb[tb.size() / 2],
                   words * 8 / (tb[tb.size() / 2] * 1e-3) / 1e9, ta[ta.size() / 2], words * 8 / (ta[ta.size() / 2] * 1e-3) / 1e9, (tb[tb.size() / 2] / ta[ta.size() / 2] - 1) * 100, bad);
            CHECK(hipMemset(out2, 0, ow * 8));
        }
    }
#endif
    if (getenv("B2B")) {
        // is part of a launch's time a fixed cost per launch?  N launches queued back to back (no host wait in between) against N x one launch
        for (int nl : { 1, 2, 4 }) {
            std::vector<float> t;
            for (int rep = 0; rep < 8; rep++) {
                CHECK(hipEventRecord(e0));
                for (int k = 0; k < nl; k++) bench_mac(lv, 3, dj, n, (int)jobs.size(), 0);
                CHECK(hipEventRecord(e1)); CHECK(hipDeviceSynchronize());
                float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
                if (rep >= 2) t.push_back(ms);
            }
            std::sort(t.begin(), t.end());
            printf("%d launches back to back: median %.3f ms = %.3f ms per launch (%.0f GB/s)\n", nl, t[t.size() / 2], t[t.size() / 2] / nl, words * 8 / (t[t.size() / 2] / nl * 1e-3) / 1e9);
        }
    }
    if (getenv("KARA")) {
        // three-product accumulation: same jobs, separate output, bit-compared with the four-product form; A B A B timing
        u64 *out2; CHECK(hipMalloc(&out2, (size_t)streams * 2 * L * n * 8));
        std::vector<MacJob> jobs2 = jobs;
        for (size_t x = 0; x < jobs2.size(); x++) for (int g = 0; g < MAC_G; g++) jobs2[x].out[g] = out2 + (jobs[x].out[g] - out);
        MacJob *dj2; CHECK(hipMalloc(&dj2, jobs2.size() * sizeof(MacJob))); CHECK(hipMemcpy(dj2, jobs2.data(), jobs2.size() * sizeof(MacJob), hipMemcpyHostToDevice));
        std::vector<float> ta, tb;
        for (int rep = 0; rep < 24; rep++) {
            float ms;
            CHECK(hipEventRecord(e0)); bench_mac(lv, 3, dj, n, (int)jobs.size(), 0, false); CHECK(hipEventRecord(e1)); CHECK(hipDeviceSynchronize());
            CHECK(hipEventElapsedTime(&ms, e0, e1)); if (rep >= 4) ta.push_back(ms);
            CHECK(hipEventRecord(e0)); bench_mac(lv, 3, dj2, n, (int)jobs2.size(), 0, true); CHECK(hipEventRecord(e1)); CHECK(hipDeviceSynchronize());
            CHECK(hipEventElapsedTime(&ms, e0, e1)); if (rep >= 4) tb.push_back(ms);
        }
        std::sort(ta.begin(), ta.end()); std::sort(tb.begin(), tb.end());
        printf("four products : min %.3f ms (%.0f GB/s)  median %.3f ms (%.0f GB/s)\n", ta[0], words * 8 / (ta[0] * 1e-3) / 1e9, ta[ta.size() / 2], words * 8 / (ta[ta.size() / 2] * 1e-3) / 1e9);
        printf("three products: min %.3f ms (%.0f GB/s)  median %.3f ms (%.0f GB/s)\n", tb[0], words * 8 / (tb[0] * 1e-3) / 1e9, tb[tb.size() / 2], words * 8 / (tb[tb.size() / 2] * 1e-3) / 1e9);
        const size_t ow = (size_t)streams * 2 * L * n;
        std::vector<u64> h1(ow), h2(ow);
        CHECK(hipMemcpy(h1.data(), out, ow * 8, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(h2.data(), out2, ow * 8, hipMemcpyDeviceToHost));
        size_t bad = 0; for (size_t x = 0; x < ow; x++) bad += h1[x] != h2[x];
        printf("three vs four products: %zu of %zu output words differ\n", bad, ow);
        if (getenv("TERMS")) return 0;
    }
#ifndef MACBENCH_PLAIN
    if (getenv("RING")) {
        // LDS-DMA ring variant: same jobs, separate output, bit-compared with k_mac's
        u64 *out2; CHECK(hipMalloc(&out2, (size_t)streams * 2 * L * n * 8));
        std::vector<MacJob> jobs2 = jobs;
        for (size_t x = 0; x < jobs2.size(); x++) for (int g = 0; g < MAC_G; g++) jobs2[x].out[g] = out2 + (jobs[x].out[g] - out);
        MacJob *dj2; CHECK(hipMalloc(&dj2, jobs2.size() * sizeof(MacJob))); CHECK(hipMemcpy(dj2, jobs2.data(), jobs2.size() * sizeof(MacJob), hipMemcpyHostToDevice));
        for (unsigned nt = 0; nt < 2; nt++) {
            std::vector<float> t;
            for (int rep = 0; rep < 16; rep++) {
                CHECK(hipEventRecord(e0)); launch_mac_ring(lv, 3, dj2, n, (int)jobs2.size(), 0, nt, getenv("RING_D") ? atoi(getenv("RING_D")) : 3, getenv("RING_LDS_KB") ? atoi(getenv("RING_LDS_KB")) * 1024 : 0); CHECK(hipEventRecord(e1)); CHECK(hipDeviceSynchronize());
                float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
                if (rep >= 2) t.push_back(ms);
            }
            std::sort(t.begin(), t.end());
            printf("k_mac_ring<%d,T=%d> nt=%u: min %.3f ms (%.0f GB/s)  median %.3f ms (%.0f GB/s)  max %.3f\n", MAC_G, APSU_MAC_RING_T, nt,
                   t[0], words * 8 / (t[0] * 1e-3) / 1e9, t[t.size() / 2], words * 8 / (t[t.size() / 2] * 1e-3) / 1e9, t.back());
        }
        const size_t ow = (size_t)streams * 2 * L * n;
        std::vector<u64> h1(ow), h2(ow);
        CHECK(hipMemcpy(h1.data(), out, ow * 8, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(h2.data(), out2, ow * 8, hipMemcpyDeviceToHost));
        size_t bad = 0; for (size_t x = 0; x < ow; x++) bad += h1[x] != h2[x];
        printf("ring vs k_mac: %zu of %zu output words differ\n", bad, ow);
        // once more k_mac, after the ring runs (same clocks / thermal state)
        std::vector<float> t;
        for (int rep = 0; rep < 12; rep++) { CHECK(hipEventRecord(e0)); bench_mac(lv, 3, dj, n, (int)jobs.size(), 0); CHECK(hipEventRecord(e1)); CHECK(hipDeviceSynchronize()); float ms; CHECK(hipEventElapsedTime(&ms, e0, e1)); t.push_back(ms); }
        std::sort(t.begin(), t.end());
        printf("k_mac again: min %.3f median %.3f\n", t[0], t[t.size() / 2]);
    }
#endif
    if (!getenv("MORPH") || MAC_G != 4) return 0;
    for (int rep = 0; rep < 2; rep++) {
#define MORPH(M, NAME) { CHECK(hipEventRecord(e0)); hipLaunchKernelGGL((k_morph<M>), dim3(16, 3, (unsigned)jobs.size() * 2), dim3(256), 0, 0, dj, n, out); CHECK(hipEventRecord(e1)); CHECK(hipDeviceSynchronize()); float ms; CHECK(hipEventElapsedTime(&ms, e0, e1)); if (rep) printf("%-40s %.3f ms  %.0f GB/s\n", NAME, ms, words * 8 / (ms * 1e-3) / 1e9); }
        MORPH(0, "morph simple loop")
        MORPH(1, "morph unroll 4")
        MORPH(2, "morph no power loads")
        MORPH(3, "morph G=4")
    }
    return 0;
}
