// kernel_bench — the k_dup_* kernels and the sort alone: reads resident in HBM, timed with HIP events (tools/dup_bench.py builds and runs it).
// usage: kernel_bench [reads = 1048576] [read length = 10000] [rounds = 7]
// The reads: molecules with random ends of 64 bases and lengths of `read length` +- 20; about one read in ten is a further copy of a molecule (sets of 2 - 4),
// every second copy reverse complemented, every fourth with one substitution in one end.  Only the first and the last 64 bases of a read are ever written: the
// kernels read nothing else of it (the bases between stay what the allocation held), so a million reads of 10 kb are 10 GB on the device and 128 MB on the host.
// Per kernel the median (min - max) of `rounds` launches; the signatures and the report of the first 512 reads — a closed world: the copies of its molecules lie
// inside it — are compared with the host rule.  Then k_dup_verify on one full bucket of 512, three ways: 512 reads that share both minimizers (a planted A x 12,
// whose hash is 0) and nothing else, so every pair passes the group and the length clause and fails the first distance of either strand (2 distances = 4 walks a
// pair); the same with one head window for all, so the same strand fails at its second distance (3 distances = 6 walks a pair); and 512 identical reads (2
// distances = 4 walks a pair, and every pair a union).  Then the two host calls on one thread, for scale.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static std::string g_err;
void ccsx_set_error(const std::string &s) { g_err = s; }
#include "../../ccs_amd/csrc/ccsx_dup.hip"
#include "../../ccs_amd/csrc/ccsx_barcode_api.cpp"
#include "../../ccs_amd/csrc/ccsx_dup_api.cpp"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static uint64_t rng_state = 0x2545f4914f6cdd1dull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }
constexpr int E = 64;                                                // bases of an end that are materialised

struct Ends { uint8_t head[E], tail[E]; int32_t len; };
// the two ends of every read to their places: byte j of read z's head to seq[off[z] + j], of its tail to seq[off[z] + len[z] - E + j]; len[z] >= 2 E
__global__ void k_place(uint8_t *seq, const int64_t *off, const int32_t *len, const uint8_t *heads, const uint8_t *tails, int n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t z = i / (2 * E);
    const int j = (int)(i % (2 * E));
    if (z >= (size_t)n) return;
    if (j < E) seq[off[z] + j] = heads[z * E + j];
    else seq[off[z] + len[z] - E + (j - E)] = tails[z * E + (j - E)];
}
static Ends rc_of(const Ends &a)
{
    Ends b; b.len = a.len;
    for (int i = 0; i < E; ++i) { b.head[i] = (uint8_t)(3 - a.tail[E - 1 - i]); b.tail[i] = (uint8_t)(3 - a.head[E - 1 - i]); }
    return b;
}

struct Timer {
    hipEvent_t e0, e1; hipStream_t s; std::vector<double> us;
    template <typename F> int run(int rounds, F f)                   // one warm-up, then `rounds` timed launches
    {
        us.clear();
        for (int r = 0; r <= rounds; ++r) {
            CK(hipEventRecord(e0, s)); f(); CK(hipGetLastError()); CK(hipEventRecord(e1, s)); CK(hipEventSynchronize(e1));
            float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
            if (r) us.push_back(ms * 1e3);
        }
        std::sort(us.begin(), us.end());
        return 0;
    }
    void line(const char *what) const { printf("%-62s median %10.1f us (min %.1f - max %.1f) over %zu launches\n", what, us[us.size() / 2], us.front(), us.back(), us.size()); }
};

// device buffers of a clustering of n signatures
struct Cluster {
    DupClusterParams P{};
    int alloc(int n, const ccsx_dup_opts &o)
    {
        P.n = n; P.opts = o; P.sort_tmp_bytes = ccsx_dup_sort_bytes(n);
        CK(hipMalloc((void **)&P.sig, (size_t)n * sizeof(ccsx_dup_sig)));
        for (int k = 0; k < 2; ++k) { CK(hipMalloc((void **)&P.key[k], (size_t)n * 8)); CK(hipMalloc((void **)&P.idx[k], (size_t)n * 4)); }
        CK(hipMalloc(&P.sort_tmp, P.sort_tmp_bytes + 16)); CK(hipMalloc((void **)&P.list, (size_t)(1 + n / 2) * 4)); CK(hipMalloc((void **)&P.rep, (size_t)n * 16));
        return 0;
    }
};

int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 1 << 20, L = argc > 2 ? atoi(argv[2]) : 10000, rounds = argc > 3 ? atoi(argv[3]) : 7, CHECK = 512;
    if (n < 1024 || n > CCSX_DUP_MAX_READS || L < 1000 || rounds < 1) { fprintf(stderr, "usage: kernel_bench [reads >= 1024] [read length >= 1000] [rounds]\n"); return 2; }
    ccsx_dup_opts o; ccsx_dup_opts_default(&o);
    const int64_t stride = L + 32;                                   // (room for the longest read)
    std::vector<Ends> ends((size_t)n);
    long copies = 0;
    auto fill = [&](int lo, int hi) {                                // reads lo .. hi - 1: molecules and their copies, the copies inside the range
        for (int z = lo; z < hi;) {
            Ends m; for (int i = 0; i < E; ++i) { m.head[i] = (uint8_t)(rnd() & 3); m.tail[i] = (uint8_t)(rnd() & 3); }
            m.len = L - 20 + (int32_t)(rnd() % 41);
            ends[z++] = m;
            if (rnd() % 25 == 0)                                     // one molecule in 25 has 1 - 3 copies more: about one read in ten is in a set
                for (int c = 1 + (int)(rnd() % 3); c > 0 && z < hi; --c, ++copies) {
                    Ends d = m; d.len += (int32_t)(rnd() % 5);
                    if (rnd() % 4 == 0) d.head[rnd() % E] ^= 1;
                    ends[z++] = (rnd() & 1) ? rc_of(d) : d;
                }
        }
    };
    fill(0, CHECK); fill(CHECK, n);
    std::vector<uint8_t> heads((size_t)n * E), tails((size_t)n * E);
    std::vector<int64_t> off((size_t)n);
    std::vector<int32_t> len((size_t)n);
    for (int z = 0; z < n; ++z) { memcpy(&heads[(size_t)z * E], ends[z].head, E); memcpy(&tails[(size_t)z * E], ends[z].tail, E); off[z] = z * stride; len[z] = ends[z].len; }
    uint8_t *d_seq; int64_t *d_off; int32_t *d_len;
    CK(hipMalloc((void **)&d_seq, (size_t)n * stride)); CK(hipMalloc((void **)&d_off, (size_t)n * 8)); CK(hipMalloc((void **)&d_len, (size_t)n * 4));
    CK(hipMemcpy(d_off, off.data(), (size_t)n * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(d_len, len.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    {
        uint8_t *d_heads, *d_tails;
        CK(hipMalloc((void **)&d_heads, heads.size())); CK(hipMalloc((void **)&d_tails, tails.size()));
        CK(hipMemcpy(d_heads, heads.data(), heads.size(), hipMemcpyHostToDevice)); CK(hipMemcpy(d_tails, tails.data(), tails.size(), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_place, dim3((unsigned)(((size_t)n * 2 * E + 255) / 256)), dim3(256), 0, 0, d_seq, d_off, d_len, d_heads, d_tails, n);
        CK(hipGetLastError()); CK(hipDeviceSynchronize());
        CK(hipFree(d_heads)); CK(hipFree(d_tails));
    }
    Timer T; CK(hipStreamCreateWithFlags(&T.s, hipStreamNonBlocking)); CK(hipEventCreate(&T.e0)); CK(hipEventCreate(&T.e1));
    Cluster C; if (C.alloc(n, o)) return 1;
    DupClusterParams &P = C.P;
    DupSignParams S{}; S.n = n; S.opts = o; S.seq = d_seq; S.seq_off = d_off; S.seq_len = d_len; S.sig = const_cast<ccsx_dup_sig *>(P.sig);
    printf("%d reads of %d +- 20 bases, %ld of them further copies of a molecule (sets of 2 - 4); window %d, kmer %d, max_dist_pct %d, max_len_diff_pct %d\n", n, L, copies,
           o.window, o.kmer, o.max_dist_pct, o.max_len_diff_pct);
    const unsigned blocks = (unsigned)((n + 255) / 256), grid = (unsigned)std::min(2048, std::max(1, n / 2));
    if (T.run(rounds, [&] { ccsx_dup_sign_launch(S, T.s); })) return 1;
    T.line("k_dup_sign");
    if (T.run(rounds, [&] { hipLaunchKernelGGL(k_dup_keys, dim3(blocks), dim3(256), 0, T.s, P); })) return 1;
    T.line("k_dup_keys");
    if (T.run(rounds, [&] { size_t b = P.sort_tmp_bytes; (void)rocprim::radix_sort_pairs(P.sort_tmp, b, P.key[0], P.key[1], P.idx[0], P.idx[1], (size_t)n, 0u, 64u, T.s); })) return 1;
    T.line("radix sort of (64-bit key, read) pairs");
    if (T.run(rounds, [&] { (void)hipMemsetAsync(P.list, 0, 4, T.s); hipLaunchKernelGGL(k_dup_buckets, dim3(blocks), dim3(256), 0, T.s, P); })) return 1;
    T.line("k_dup_buckets (with the list counter's memset)");
    int32_t listed = 0; CK(hipMemcpy(&listed, P.list, 4, hipMemcpyDeviceToHost));
    if (T.run(rounds, [&] { hipLaunchKernelGGL(k_dup_verify, dim3(grid), dim3(NT), 0, T.s, P); })) return 1;
    char what[128]; snprintf(what, sizeof what, "k_dup_verify (%d buckets of 2 or more, %u workgroups)", listed, grid);
    T.line(what);
    if (T.run(rounds, [&] { ccsx_dup_cluster_launch(P, T.s); })) return 1;
    T.line("the cluster call's four kernels and the sort, one after another");
    // the check: the first 512 reads on the host, from reads rebuilt with zeros between the ends
    std::vector<ccsx_dup_sig> sig((size_t)n);
    std::vector<int32_t> planes((size_t)n * 4);
    CK(hipMemcpy(sig.data(), P.sig, (size_t)n * sizeof(ccsx_dup_sig), hipMemcpyDeviceToHost)); CK(hipMemcpy(planes.data(), P.rep, (size_t)n * 16, hipMemcpyDeviceToHost));
    {
        std::vector<uint8_t> seq((size_t)CHECK * stride, 0);
        for (int z = 0; z < CHECK; ++z) { memcpy(&seq[(size_t)off[z]], ends[z].head, E); memcpy(&seq[(size_t)(off[z] + len[z] - E)], ends[z].tail, E); }
        std::vector<ccsx_dup_sig> hs((size_t)CHECK);
        std::vector<int32_t> hp((size_t)CHECK * 4);
        ccsx_dup_report rep{CHECK, hp.data(), hp.data() + CHECK, hp.data() + 2 * CHECK, hp.data() + 3 * CHECK};
        if (ccsx_dup_sign_reads_host(&o, seq.data(), off.data(), len.data(), CHECK, hs.data()) || ccsx_dup_cluster_host(&o, hs.data(), nullptr, nullptr, CHECK, &rep)) {
            fprintf(stderr, "host rule: %s\n", g_err.c_str()); return 1;
        }
        if (memcmp(hs.data(), sig.data(), (size_t)CHECK * sizeof(ccsx_dup_sig))) { fprintf(stderr, "the signatures of the first %d reads differ from the host rule\n", CHECK); return 1; }
        // (a read past the first 512 may share a key with one of them by chance, never a pair: its planes are compared as they are)
        for (int k = 0; k < 4; ++k)
            if (memcmp(&hp[(size_t)k * CHECK], &planes[(size_t)k * n], (size_t)CHECK * 4)) { fprintf(stderr, "plane %d of the first %d reads differs from the host rule\n", k, CHECK); return 1; }
    }
    long dups = 0, in_sets = 0, overflow = 0;
    for (int z = 0; z < n; ++z) { dups += planes[3 * (size_t)n + z]; in_sets += planes[2 * (size_t)n + z] > 1; overflow += planes[z] == CCSX_DUP_OVERFLOW; }
    printf("  %ld reads in sets of 2 or more, %ld duplicates, %ld in overflowed buckets; signatures and report of the first %d reads equal the host rule\n", in_sets, dups, overflow, CHECK);

    // ---- one full bucket of 512
    for (int kind = 0; kind < 3; ++kind) {                           // 0: unrelated, 1: one head window for all, 2: identical
        const bool identical = kind == 2;
        const int m = CCSX_DUP_MAX_BUCKET;
        std::vector<ccsx_dup_sig> fs((size_t)m);
        std::vector<uint8_t> seq((size_t)m * 200);
        std::vector<int64_t> foff((size_t)m); std::vector<int32_t> flen((size_t)m, 200);
        for (int z = 0; z < m; ++z) {
            uint8_t *c = &seq[(size_t)z * 200]; foff[z] = z * 200;
            for (int i = 0; i < 200; ++i) c[i] = identical ? (uint8_t)((i * 7 + i / 5) & 3) : (uint8_t)(rnd() & 3);
            if (!identical) { memset(c + 10, 0, 12); memset(c + 200 - 22, 3, 12); }   // A x 12 in the head, and in the reverse complement's head: both minimizers are hash(0) = 0
            if (kind == 1 && z) memcpy(c, &seq[0], 32);
        }
        if (ccsx_dup_sign_reads_host(&o, seq.data(), foff.data(), flen.data(), m, fs.data())) { fprintf(stderr, "host rule: %s\n", g_err.c_str()); return 1; }
        for (int z = 1; z < m; ++z) if (ccsx_dup_key(fs[z]) != ccsx_dup_key(fs[0])) { fprintf(stderr, "the full bucket is not one bucket\n"); return 1; }
        Cluster F; if (F.alloc(m, o)) return 1;
        CK(hipMemcpy(const_cast<ccsx_dup_sig *>(F.P.sig), fs.data(), (size_t)m * sizeof(ccsx_dup_sig), hipMemcpyHostToDevice));
        if (const char *failed = ccsx_dup_cluster_launch(F.P, T.s)) { fprintf(stderr, "launch failed: %s\n", failed); return 1; }
        CK(hipStreamSynchronize(T.s));
        if (T.run(rounds, [&] { hipLaunchKernelGGL(k_dup_verify, dim3(1), dim3(NT), 0, T.s, F.P); })) return 1;
        std::vector<int32_t> fp((size_t)m * 4), hp((size_t)m * 4);
        CK(hipMemcpy(fp.data(), F.P.rep, (size_t)m * 16, hipMemcpyDeviceToHost));
        ccsx_dup_report rep{m, hp.data(), hp.data() + m, hp.data() + 2 * m, hp.data() + 3 * m};
        const auto t0 = std::chrono::steady_clock::now();
        if (ccsx_dup_cluster_host(&o, fs.data(), nullptr, nullptr, m, &rep)) { fprintf(stderr, "host rule: %s\n", g_err.c_str()); return 1; }
        const double host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (fp != hp) { fprintf(stderr, "the full bucket's report differs from the host rule\n"); return 1; }
        long sets = 0; for (int z = 0; z < m; ++z) sets += fp[(size_t)m + z] == z;
        snprintf(what, sizeof what, "k_dup_verify, one bucket of 512 %s", kind == 2 ? "identical reads (4 walks a pair)" : kind == 1 ? "reads of one head (6 walks a pair)" : "unrelated reads (4 walks a pair)");
        T.line(what);
        printf("  130816 pairs, %ld sets; the report equals the host rule, which takes %.1f ms on one thread\n", sets, host_ms);
    }

    // ---- the host calls, for scale: one thread (the host calls are not threaded)
    {
        const int hn = std::min(n, 65536);
        std::vector<uint8_t> seq((size_t)hn * stride, 0);
        for (int z = 0; z < hn; ++z) { memcpy(&seq[(size_t)off[z]], ends[z].head, E); memcpy(&seq[(size_t)(off[z] + len[z] - E)], ends[z].tail, E); }
        std::vector<ccsx_dup_sig> hs((size_t)hn);
        auto t0 = std::chrono::steady_clock::now();
        if (ccsx_dup_sign_reads_host(&o, seq.data(), off.data(), len.data(), hn, hs.data())) return 1;
        const double sign_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::vector<int32_t> hp((size_t)n * 4);
        ccsx_dup_report rep{n, hp.data(), hp.data() + n, hp.data() + 2 * (size_t)n, hp.data() + 3 * (size_t)n};
        t0 = std::chrono::steady_clock::now();
        if (ccsx_dup_cluster_host(&o, sig.data(), nullptr, nullptr, n, &rep)) return 1;
        const double cl_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("host, one thread: ccsx_dup_sign_reads_host on %d reads %.1f ms (%.2f us a read); ccsx_dup_cluster_host on the %d signatures %.1f ms; its report %s the device's\n",
               hn, sign_ms, sign_ms * 1e3 / hn, n, cl_ms, hp == planes ? "equals" : "DIFFERS FROM");
        if (hp != planes) return 1;
    }
    return 0;
}
