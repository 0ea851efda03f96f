// psl_lm_optimize<6> of psl-slam_amd/csrc/lm_kernels.h - the Levenberg driver psl_lm_levenberg on one vertex - on scripted problems:
// sums() and chi() return what the script lists, candidate() records the step it is handed, accept() counts its calls.
// tests/test_lm_driver_cpu.py writes the scripts, builds this program under the address and undefined-behaviour sanitizers and
// compares what it records with lm_cases.levenberg on the same scripts.
//
// usage: lm_driver_host <scripts.bin> <out.bin>
//   scripts.bin: int32 K; K x { int32 iterations, nsums, nchi; double sums[nsums][28] (H 21, b 6, chi2); double chi[nchi] }
//   out.bin:     K x { int32 iterations run, accept calls, candidates, sums() calls, chi() calls; double x[candidates][6] }
#include <stdio.h>

#include <vector>

#include "../psl-slam_amd/csrc/lm_kernels.h"

namespace {

constexpr int N = 6, NACC = N * (N + 1) / 2 + N + 1;

struct Scripted {
    std::vector<double> sums_list, chi_list, xs;
    size_t sums_at = 0, chi_at = 0;
    int accepts = 0, overrun = 0;
    void sums(double* acc) {
        if ((sums_at + 1) * NACC > sums_list.size()) { overrun = 1; for (int k = 0; k < NACC; ++k) acc[k] = 0.0; return; }
        for (int k = 0; k < NACC; ++k) acc[k] = sums_list[sums_at * NACC + k];
        ++sums_at;
    }
    void candidate(double* x) { xs.insert(xs.end(), x, x + N); }
    double chi() {
        if (chi_at >= chi_list.size()) { overrun = 1; return 0.0; }
        return chi_list[chi_at++];
    }
    void accept() { ++accepts; }
};

bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: lm_driver_host <scripts.bin> <out.bin>\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "lm_driver_host: cannot open the files\n"); return 2; }
    int32_t K = 0;
    if (!rd(in, &K, sizeof K)) { fprintf(stderr, "lm_driver_host: short file\n"); return 2; }
    for (int k = 0; k < K; ++k) {
        int32_t head[3];
        if (!rd(in, head, sizeof head) || head[1] < 0 || head[2] < 0) { fprintf(stderr, "lm_driver_host: script %d: bad header\n", k); return 2; }
        Scripted P;
        P.sums_list.resize((size_t)head[1] * NACC);
        P.chi_list.resize((size_t)head[2]);
        if (!rd(in, P.sums_list.data(), P.sums_list.size() * sizeof(double)) || !rd(in, P.chi_list.data(), P.chi_list.size() * sizeof(double))) {
            fprintf(stderr, "lm_driver_host: script %d: short file\n", k);
            return 2;
        }
        const int its = psl_lm_optimize<N>(P, head[0]);
        if (P.overrun) { fprintf(stderr, "lm_driver_host: script %d asked for more values than it lists\n", k); return 3; }
        const int32_t rec[5] = {its, P.accepts, (int32_t)(P.xs.size() / N), (int32_t)P.sums_at, (int32_t)P.chi_at};
        fwrite(rec, sizeof rec, 1, out);
        fwrite(P.xs.data(), sizeof(double), P.xs.size(), out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
