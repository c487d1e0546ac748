// kernel_bench — k_represent alone: a batch resident in HBM, timed with HIP events (tools/represent_bench.py builds and runs it).
// usage: kernel_bench [ZMWs = 16384] [passes = 10] [pass length = 10000] [rounds = 7]
// Three configurations, one launch over all ZMWs per round: every ZMW polished (the kernel reads the statuses and leaves), every fourth ZMW with a single pass and
// TOO_FEW_PASSES (a subread copied), every ZMW TOO_MANY_UNUSABLE with a draft of the pass length (a draft copied).  After the first round the lengths, the report
// and the first and last bases of the first 64 written ZMWs are compared with what the rule says.  One line per configuration.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../ccs_amd/csrc/ccsx_represent.hip"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 16384, P = argc > 2 ? atoi(argv[2]) : 10, L = argc > 3 ? atoi(argv[3]) : 10000, rounds = argc > 4 ? atoi(argv[4]) : 7;
    if (n < 1 || P < 1 || P > CCSX_MAX_PASSES || L < 1 || L > 65535 || rounds < 1) { fprintf(stderr, "usage: kernel_bench [ZMWs] [passes] [pass length] [rounds]\n"); return 2; }
    const int64_t slot = L + L / 4 + 64, cap = (int64_t)n * slot;
    hipStream_t s; CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<int64_t> seq_off((size_t)n + 1);
    for (int z = 0; z <= n; ++z) seq_off[z] = (int64_t)z * slot;
    int64_t *d_seq_off; uint8_t *d_draft, *d_seq, *d_qual; float *d_raw, *d_rq, *d_ec; int32_t *d_len, *d_dlen, *d_status, *d_rep;
    CK(hipMalloc((void **)&d_seq_off, ((size_t)n + 1) * 8)); CK(hipMalloc((void **)&d_draft, (size_t)cap)); CK(hipMalloc((void **)&d_seq, (size_t)cap));
    CK(hipMalloc((void **)&d_qual, (size_t)cap)); CK(hipMalloc((void **)&d_raw, (size_t)cap * 4)); CK(hipMalloc((void **)&d_rq, (size_t)n * 4)); CK(hipMalloc((void **)&d_ec, (size_t)n * 4));
    CK(hipMalloc((void **)&d_len, (size_t)n * 4)); CK(hipMalloc((void **)&d_dlen, (size_t)n * 4)); CK(hipMalloc((void **)&d_status, (size_t)n * 4));
    CK(hipMalloc((void **)&d_rep, (size_t)n * CCSX_RP_PLANES * 4));
    CK(hipMemcpy(d_seq_off, seq_off.data(), seq_off.size() * 8, hipMemcpyHostToDevice));
    CK(hipMemset(d_draft, 0x02, (size_t)cap));
    const struct { const char *name; int single_every; int status; int draft; } configs[] = {
        {"every ZMW polished", 0, CCSX_SUCCESS, 0}, {"every fourth ZMW a single pass", 4, CCSX_SUCCESS, 0}, {"every ZMW an unpolished draft", 0, CCSX_TOO_MANY_UNUSABLE, 1}};
    for (const auto &c : configs) {
        std::vector<int32_t> read_off((size_t)n + 1, 0), status((size_t)n), dlen((size_t)n, c.draft ? L : 0);
        for (int z = 0; z < n; ++z) {
            const bool single = c.single_every && z % c.single_every == 0;
            read_off[z + 1] = read_off[z] + (single ? 1 : P);
            status[z] = single ? CCSX_TOO_FEW_PASSES : c.status;
        }
        const int R = read_off[n];
        std::vector<int64_t> base_off((size_t)R + 1);
        for (int r = 0; r <= R; ++r) base_off[r] = (int64_t)r * L + (r % 7);      // (sources at every alignment; r % 7 <= 6 bytes of slack per pass, below)
        const size_t nb = (size_t)R * L + 8;
        int32_t *d_read_off; int64_t *d_base_off; uint8_t *d_bases, *d_flags;
        CK(hipMalloc((void **)&d_read_off, ((size_t)n + 1) * 4)); CK(hipMalloc((void **)&d_base_off, ((size_t)R + 1) * 8)); CK(hipMalloc((void **)&d_bases, nb)); CK(hipMalloc((void **)&d_flags, (size_t)R));
        CK(hipMemcpy(d_read_off, read_off.data(), read_off.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(d_base_off, base_off.data(), base_off.size() * 8, hipMemcpyHostToDevice));
        CK(hipMemset(d_bases, 0x47, nb)); CK(hipMemset(d_flags, 0, (size_t)R));
        CK(hipMemcpy(d_status, status.data(), (size_t)n * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(d_dlen, dlen.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        CK(hipMemset(d_len, 0, (size_t)n * 4)); CK(hipMemset(d_seq, 0xA5, (size_t)cap));
        RepresentParams Q{};
        Q.n = n; Q.top_passes = 0; Q.subread_fallback = 0; Q.read_off = d_read_off; Q.base_off = d_base_off; Q.bases = d_bases; Q.pw = d_bases; Q.ipd = d_bases; Q.flags = d_flags;
        Q.seq_off = d_seq_off; Q.draft = d_draft; Q.draft_len = d_dlen; Q.status = d_status; Q.out_len = d_len; Q.out_rq = d_rq; Q.out_ec = d_ec; Q.out_seq = d_seq;
        Q.out_qual = d_qual; Q.out_raw = d_raw; Q.out_kin = nullptr; Q.kin_plane = 0; Q.rep = d_rep;
        // (a pass has L + 1 bases, or L - 6 where r % 7 wraps: never more than its slot; the last one ends at R * L + 6 < nb)
        std::vector<double> us;
        long long written = 0;
        for (int r = 0; r <= rounds; ++r) {                          // round 0 warms up and is checked
            CK(hipEventRecord(e0, s));
            if (const char *failed = ccsx_represent_launch(Q, s)) { fprintf(stderr, "launch failed: %s\n", failed); return 1; }
            CK(hipEventRecord(e1, s));
            CK(hipEventSynchronize(e1));
            float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
            if (r > 0) { us.push_back(ms * 1e3); continue; }
            std::vector<int32_t> len((size_t)n), rep((size_t)n * 2);
            CK(hipMemcpy(len.data(), d_len, (size_t)n * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(rep.data(), d_rep, rep.size() * 4, hipMemcpyDeviceToHost));
            int checked = 0;
            for (int z = 0; z < n; ++z) {
                const bool single = c.single_every && z % c.single_every == 0;
                const int cls = single ? CCSX_REPRESENT_SUBREAD : (c.draft ? CCSX_REPRESENT_DRAFT : CCSX_REPRESENT_POLISHED);
                const int want = single ? (int)(base_off[read_off[z] + 1] - base_off[read_off[z]]) : (c.draft ? L : 0);
                if (rep[z] != cls || rep[(size_t)n + z] != (single ? 0 : -1) || len[z] != want) { fprintf(stderr, "%s: ZMW %d: class %d pass %d length %d\n", c.name, z, rep[z], rep[(size_t)n + z], len[z]); return 1; }
                written += want;
                if (want > 0 && checked < 64) {
                    uint8_t ends[2], past;
                    CK(hipMemcpy(&ends[0], d_seq + seq_off[z], 1, hipMemcpyDeviceToHost)); CK(hipMemcpy(&ends[1], d_seq + seq_off[z] + want - 1, 1, hipMemcpyDeviceToHost));
                    CK(hipMemcpy(&past, d_seq + seq_off[z] + want, 1, hipMemcpyDeviceToHost));
                    const uint8_t b = single ? (0x47 & 3) : 0x02;
                    if (ends[0] != b || ends[1] != b || past != 0xA5) { fprintf(stderr, "%s: ZMW %d: bases %d %d, behind the end %d\n", c.name, z, ends[0], ends[1], past); return 1; }
                    ++checked;
                }
            }
        }
        std::sort(us.begin(), us.end());
        const double med = us[us.size() / 2], bytes = (double)written * 7.0;     // read 1, written seq 1 + qual 1 + raw_qv 4
        printf("k_represent alone: %d ZMWs x %d passes x %d bases, %s: median %8.1f us (min %.1f, max %.1f) over %d rounds; %lld bases written", n, P, L, c.name, med, us.front(),
               us.back(), rounds, written);
        if (written) printf(" = %.0f GB/s of copy and fill", bytes / (med * 1e3));
        printf("; lengths, report and the ends of the first 64 written sequences as the rule says\n");
        CK(hipFree(d_read_off)); CK(hipFree(d_base_off)); CK(hipFree(d_bases)); CK(hipFree(d_flags));
    }
    return 0;
}
